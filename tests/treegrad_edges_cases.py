"""Shared inputs of the edge tests of phylo_trees_grad_rates and phylo_trees_grad_model (DESIGN.md sections 13b, 13c) where their
own suites stop: items of several strips, 129 to 512 taxa in every shape, a workgroup's second 512-taxon item, site values at the
floor of the double range.  The trees, alignments and places are those of trees_edges_cases.py; here are the mixtures and
directions, the restatements' error against 50 digits on deep trees, and the near-floor bound of drate and dweight.
test_treegrad_edges_cpu.py holds every case to its precondition from the NumPy restatements alone; the two device files assert
them again before they compare anything."""
import contextlib
import ctypes
import ctypes.util

import numpy as np

import treegrad_model_ref as MR
import treegrad_rates_ref as TRR
import treegrad_ref as TR
import trees_edges_cases as EC
from phylo_amd import modelfit
from phylo_amd import rates as R
from treegrad_cases import branch_matrices
from treegrad_rates_cases import E_REF_RATES, MIX_I_G4, TOL_RATES, category_matrices

PRIOR = EC.PRIOR
C16 = R.rate_model(0.7, 15, 0.05)                                          # test_gpu_treegrad_rates.py's 'C16': the LDS maximum
MIX_SLOW_FAST = (np.array([0.0, 0.3, 1.0, 8.0]), np.array([0.1, 0.3, 0.3, 0.3]))   # the floor's second mixture: another small category
T_STRIPS = 7


# ---- A. items of several strips (rates) -------------------------------------------------------------------------------------------
def strips(N, S, mix='C5', **kw):
    return dict(N=N, S=S, mix=mix, **kw)


# the default tile holds all S sites: one item of ceil(S / 128) strips of two site steps of 64 lanes
STRIPS = {
    'N5-S300-gaps': strips(5, 300, gaps=True),                             # three strips, the last with 44 live lanes and an empty second step
    'N12-S600-gaps': strips(12, 600, gaps=True),                           # five strips, the last with a second step of 24 lanes
    'N12-S200-generic': strips(12, 200, generic=True),                     # two strips, a second step of 8 lanes
    'N12-S300-C16': strips(12, 300, mix='C16'),
    'N12-S130': strips(12, 130),                                           # a full strip, then one with two live lanes in its first step
    'N12-S66': strips(12, 66),                                             # one strip whose second step has two live lanes
    'N12-S128': strips(12, 128),                                           # one strip, exactly full
}
MIXTURES = {'C5': MIX_I_G4, 'C16': C16}


# ---- B, C. the restatements against 50 digits above 128 taxa ----------------------------------------------------------------------
# Measured by test_treegrad_edges_cpu.py::test_reference_against_mpmath_big on tree 0 of caterpillar-N512, random-N257 and
# balanced-N129 at four sites each (the first, the last and the first two variable ones between them), in the units of
# E_REF_RATES and E_REF_MODEL -- (scale + |value|) 2^-53 over the sums of those four sites.
#   rates (MIX_I_G4)     grad   curv   drate  dweight                     model (P = 4)   dtheta  dprior
#   caterpillar-N512     15.95  62.72  13.43  22.63  (raw 336.1, 22844)                    2.154   0.567
#   random-N257           6.10  18.48   1.83   2.47                                        1.628   1.886
#   balanced-N129         4.01  16.42   1.11   2.37                                        1.128   0.734
# The error of the rate call grows with a caterpillar's depth, as section 14's did: E_REF_RATES_BIG is above E_REF_RATES = 7.6 and
# parts B and C of the rate call use TOL_RATES_BIG.  The model call's stays below E_REF_MODEL = 2.7: TOL_MODEL stands unchanged.
# drate and dweight are measured net of section 13b's absolute allowance (floor_excess' terms, over every site): at site 64 of
# caterpillar-N512 category 1 has f_1 = 2^-1036, a subnormal with 38 bits, beside m = 2^-643, and at sites 0 to 2 it is zero, so
# over these four sites -- none of them constant -- dweight_1 = sum_s f_1 / m is made of that one value and its raw error is 22844
# units of itself.  Over the case's 65 sites the sum is 1.9e-93 and made of normal numbers.  The test asserts that the measured
# values stay at or below the recorded ones, and the rate call's above half of it.
E_REF_RATES_BIG = 63.0
E_REF_MODEL_BIG = 2.2
MP_CASES = ('caterpillar-N512', 'random-N257', 'balanced-N129')
TOL_RATES_BIG = 8 * max(E_REF_RATES, E_REF_RATES_BIG) * 2.0 ** -53
TOL_MODEL_BIG = 8 * max(MR.E_REF_MODEL, E_REF_MODEL_BIG) * 2.0 ** -53


def close_tol(name, got, ref, scale, tol):
    """test_gpu_treegrad_rates.close with the tolerance an argument (parts B and C: TOL_RATES_BIG, TOL_MODEL_BIG)"""
    bound = scale + np.abs(ref)
    with np.errstate(invalid='ignore', divide='ignore'):
        err = np.where(bound == 0, np.where(got == 0, 0.0, np.inf), np.abs(got - ref) / bound)
    print("%s: worst |device - reference| / (scale + |value|) = %.3g (tolerance %.3g)" % (name, np.nanmax(err), tol))
    assert np.isfinite(got).all(), name
    assert (err <= tol).all(), (name, float(np.nanmax(err)), tol)


def close_all_big(name, got, ref):
    """got = (loglik, grad, curv, drate, dweight) of the device, ref the restatement's dict: test_gpu_treegrad_rates.close_all
    at TOL_RATES_BIG"""
    np.testing.assert_allclose(got[0], ref['loglik'], rtol=1e-12, atol=0)
    close_tol(name + " grad", got[1], ref['grad'], ref['scale'], TOL_RATES_BIG)
    close_tol(name + " curv", got[2], ref['curv'], ref['scale'], TOL_RATES_BIG)
    close_tol(name + " drate", got[3], ref['drate'], ref['drate_scale'], TOL_RATES_BIG)
    close_tol(name + " dweight", got[4], ref['dweight'], ref['dweight'], TOL_RATES_BIG)


def model_directions(P, Q, seed=1):
    """P = 4: one direction of the row-softmax, Q itself and two random ones; P = 1, 12, 16: test_gpu_treegrad_model.directions'
    sets (built here as there, so that the CPU file needs no device test's module state)"""
    rng = np.random.default_rng(seed)
    d = np.concatenate([modelfit.q_directions(rng.normal(size=(4, 4))), Q[None], rng.normal(size=(3, 4, 4))])
    return np.ascontiguousarray({1: d[5:6], 4: d[[5, 12, 13, 14]], 12: d[:12], 16: d}[P])


def mp_sites(g):
    """the first site, the first two variable ones after it, the last"""
    S = g.shape[1]
    variable = [s for s in range(1, S - 1) if (g[:, s] != g[0, s]).any()]
    return [0] + variable[:2] + [S - 1]


def measure_rates_big(mp, name):
    """the worst |restatement - 50-digit value| of grad, curv, drate, dweight of tree 0 over the case's mp_sites, in units of
    (scale + |value|) 2^-53 (test_treegrad_rates_cpu.py::test_reference_against_mpmath's accounting)"""
    mpf = mp.mpf
    g, child, blen, Q = EC.big_case(name)
    c, b = child[0], blen[0]
    gs = np.ascontiguousarray(g[:, mp_sites(g)])
    N, S = gs.shape[0], gs.shape[1]
    rates, weights = MIX_I_G4
    C = rates.size
    M = category_matrices(Q, b, rates)
    ref = TRR.tree_grad_rates(c, M, Q, PRIOR, gs, b, rates, weights)
    assert np.isfinite(ref['grad']).all() and (ref['m'] >= EC.ROOMY).all()
    cv = lambda a: [cv(v) for v in a] if np.ndim(a) else mpf(float(a))
    Mm, Qm, pm, bm, rm, wm = cv(M), cv(Q), cv(PRIOR), cv(b), cv(rates), cv(weights)
    G = [[mpf(0), mpf(0)] for _ in range(N - 1)]
    Cv = [[mpf(0), mpf(0)] for _ in range(N - 1)]
    Dr, Dw = [mpf(0)] * C, [mpf(0)] * C
    for s in range(S):
        m, a1, a2, dr, f = TRR.site_terms_rates(c.tolist(), Mm, Qm, pm, cv(gs[:, s]), bm, rm, wm, mpf(0))
        for i in range(N - 1):
            for sd in range(2):
                G[i][sd] += a1[i][sd] / m
                Cv[i][sd] += a2[i][sd] / m - (a1[i][sd] / m) ** 2
        for k in range(C):
            Dr[k] += dr[k] / m
            Dw[k] += f[k] / m
    worst = {'grad': 0.0, 'curv': 0.0, 'drate': 0.0, 'dweight': 0.0}

    def err(key, val, exact, scale):
        unit = (mpf(float(scale)) + abs(exact)) * mpf(2) ** -53
        if unit > 0:
            worst[key] = max(worst[key], float(abs(mpf(float(val)) - exact) / unit))
        else:
            assert val == 0

    for i in range(N - 1):
        for sd in range(2):
            err('grad', ref['grad'][i, sd], G[i][sd], ref['scale'][i, sd])
            err('curv', ref['curv'][i, sd], Cv[i][sd], ref['scale'][i, sd])
    worst['drate_raw'], worst['dweight_raw'] = 0.0, 0.0
    per_m = sum((mpf(2) ** -1075 / mpf(float(v)) for v in ref['m']), mpf(0))
    blen_sum = sum((v for row in bm for v in row), mpf(0))
    for k in range(C):
        err('drate_raw', ref['drate'][k], Dr[k], ref['drate_scale'][k])
        err('dweight_raw', ref['dweight'][k], Dw[k], ref['dweight'][k])
        # net of section 13b's absolute allowance for a category whose own terms are subnormal beside an m in range (K_R, K_W below)
        unit_r = (mpf(float(ref['drate_scale'][k])) + abs(Dr[k])) * mpf(2) ** -53
        unit_w = 2 * abs(Dw[k]) * mpf(2) ** -53
        over_r = abs(mpf(float(ref['drate'][k])) - Dr[k]) - K_R * per_m * blen_sum * wm[k]
        over_w = abs(mpf(float(ref['dweight'][k])) - Dw[k]) - K_W * per_m
        if over_r > 0:
            worst['drate'] = max(worst['drate'], float(over_r / unit_r))
        if over_w > 0:
            worst['dweight'] = max(worst['dweight'], float(over_w / unit_w))
    worst['subnormal_f'] = int(((ref['f'] > 0) & (ref['f'] < 2.0 ** -1022)).sum())
    return worst


def exact_direction_matrices(mp, Q, dirs):
    """exact_D(p, t) -> L(Q t, dirs[p] t) [4][4] at the working precision, through Q's eigenvectors at twice the digits:
    L = V (G o Phi) V^-1 with G = V^-1 E V, Phi_ii = t e^(l_i t), Phi_ij = (e^(l_i t) - e^(l_j t)) / (l_i - l_j).  One
    eigendecomposition serves every branch, where mpmath.expm of the 8 x 8 block matrix costs 30 ms a branch and direction;
    the first two calls with t > 0 are checked against that expm."""
    mpf = mp.mpf
    dps = mp.mp.dps
    checked = [0]
    with mp.workdps(2 * dps + 10):
        Qm = mp.matrix([[mpf(float(v)) for v in row] for row in Q])
        lam, V = mp.eig(Qm)
        gaps = [abs(lam[i] - lam[j]) for i in range(4) for j in range(i)]
        assert min(gaps) > mpf(10) ** -3, gaps                             # distinct eigenvalues: the divided differences are safe
        Vi = V ** -1
        G = [Vi * mp.matrix([[mpf(float(v)) for v in row] for row in E]) * V for E in dirs]

    def by_expm(p, t):
        B = mp.zeros(8, 8)
        for i in range(4):
            for j in range(4):
                B[i, j] = B[4 + i, 4 + j] = mpf(float(Q[i, j])) * mpf(float(t))
                B[i, 4 + j] = mpf(float(dirs[p][i, j])) * mpf(float(t))
        X = mp.expm(B)
        return [[X[i, 4 + j] for j in range(4)] for i in range(4)]

    def exact_D(p, t):
        if t == 0.0:
            return [[mpf(0)] * 4 for _ in range(4)]
        with mp.workdps(2 * dps + 10):
            tm = mpf(float(t))
            ex = [mp.exp(lam[i] * tm) for i in range(4)]
            H = mp.matrix(4, 4)
            for i in range(4):
                for j in range(4):
                    H[i, j] = G[p][i, j] * (tm * ex[i] if i == j else (ex[i] - ex[j]) / (lam[i] - lam[j]))
            X = V * H * Vi
            out = [[+mp.re(X[i, j]) for j in range(4)] for i in range(4)]
            assert max(abs(mp.im(X[i, j])) for i in range(4) for j in range(4)) < mpf(10) ** -(dps + 20)
        if checked[0] < 2:
            checked[0] += 1
            ref = by_expm(p, t)
            assert max(abs(out[i][j] - ref[i][j]) for i in range(4) for j in range(4)) < mpf(10) ** -(dps - 8)
        return out

    return exact_D


def measure_model_big(mp, name, P=4):
    """the same for dtheta and dprior (test_treegrad_model_cpu.py::test_reference_against_mpmath's accounting: the exact D from
    mpmath.expm of [[A, E], [0, A]] on the same doubles Q, dirs, t)"""
    mpf = mp.mpf
    g, child, blen, Q = EC.big_case(name)
    c, b = child[0], blen[0]
    gs = np.ascontiguousarray(g[:, mp_sites(g)])
    N, S = gs.shape[0], gs.shape[1]
    dirs = model_directions(P, Q)
    M = branch_matrices(Q, b)
    D = MR.direction_matrices(Q, dirs, b)
    _, dth, dpr, sc_t, sc_p = MR.tree_grad_model(c, M, D, PRIOR, gs)
    assert np.isfinite(dth).all()
    cv = lambda a: [cv(v) for v in a] if np.ndim(a) else mpf(float(a))
    exact_D = exact_direction_matrices(mp, Q, dirs)
    Dm = [[[exact_D(p, b[i, sd]) for p in range(P)] for sd in range(2)] for i in range(N - 1)]
    Mm, pm = cv(M), cv(PRIOR)
    Th, Pr = [mpf(0)] * P, [mpf(0)] * 4
    for s in range(S):
        L, tot, _, xr = MR.site_terms_model(c.tolist(), Mm, Dm, pm, cv(gs[:, s]), mpf(0))
        for p in range(P):
            Th[p] += tot[p] / L
        for j in range(4):
            Pr[j] += xr[j] / L
    unit = lambda scale, exact: (mpf(float(scale)) + abs(exact)) * mpf(2) ** -53
    worst_t = max(float(abs(mpf(float(dth[p])) - Th[p]) / unit(sc_t[p], Th[p])) for p in range(P))
    worst_p = max(float(abs(mpf(float(dpr[j])) - Pr[j]) / unit(sc_p[j], Pr[j])) for j in range(4))
    return {'dtheta': worst_t, 'dprior': worst_p}


# ---- D. the floor: drate and dweight where a category's factor is subnormal beside an m in range ---------------------------------
# The floor rule guards 1 / m, not a category's own terms.  Where m lies in [2^-1020, 2^-1000) a category whose share f_c / m is
# small has a subnormal f_c, and a subnormal's rounding is absolute: half the smallest subnormal, 2^-1075, per operation, whatever
# the value's size.  Counted in the code, not fitted:
#   K_W = 5: pk_site_lik is one product and three fma (4 roundings) on pr[j] o[j], and o[j] = el[j] er[j] is one rounding more
#            per component, which enters with the weights pr[j] that sum to one.  So f_c carries at most 5 2^-1075 of absolute
#            error from operations at its own scale, and one site's term f_c / m of dweight_c at most K_W 2^-1075 / m_s.
#   K_R = 35: ptg_xDg makes four t[k], each four products and three sums (7 roundings), then four products x[k] t[k] and three
#            sums (7 more); with x[k] <= 1 that is at most 4 7 + 7 = 35 roundings of 2^-1075 each on one branch's D1, and one
#            site's term of drate_c, sum_b (blen_b w_c) D1_{c,b} / m, carries at most K_R 2^-1075 sum_b blen_b w_c / m_s.
# What feeds these chains from nodes between the join of the two scaled leaves and the root is rounded at the same scale and is
# NOT counted; neither is it needed.  Measured by test_treegrad_edges_cpu.py::test_the_finding_is_inside_its_bound_and_outside_the_plain_tolerance (restatement,
# scaled against unscaled, every in-range place, both mixtures): the worst |difference| / bound is 0.328 (WORST_RATIO; dweight at
# at-the-floor under MIX_I_G4), while against TOL_RATES alone the same differences are 3.7e3 (drate) and 9.8e4 (dweight) units
# of (scale + |value|) 2^-53 where TOL_RATES is 61 of them.
K_W = 5
K_R = 35


@contextlib.contextmanager
def hardware_fma():
    """treegrad_ref.fma emulates the device's fma only where |a b| > 1e-290 (its docstring): below that the product's error term
    underflows and the emulation is an ordinary chain of rounded operations.  Beside an m in range that is an ulp of a SUBNORMAL
    category factor, the size of the whole finding above, and the device -- whose fma rounds once -- is then further from the
    restatement than from the truth (measured on the device at at-the-floor under +I+G4: dweight_1 off by 2.0e-13 of itself,
    1.8e3 units).  Inside this context the elements with 0 < |a b| < 1e-280 take the C library's correctly rounded fma instead;
    every other element keeps the emulation, so results in range keep their bits (test_treegrad_edges_cpu.py asserts it)."""
    libm = ctypes.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    emulated = TR.fma

    def fma(a, b, c):
        a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
        with np.errstate(all='ignore'):
            out = np.array(emulated(a, b, c))
            low = (np.abs(a * b) < 1e-280) & (a != 0) & (b != 0) & np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
        if low.any():
            out[low] = [libm.fma(x, y, z) for x, y, z in zip(a[low].tolist(), b[low].tolist(), c[low].tolist())]
        return out

    TR.fma = fma
    try:
        yield
    finally:
        TR.fma = emulated
WORST_RATIO = 0.33


def floor_excess(m_scaled, blen, weights):
    """(extra_drate [T][C], extra_dweight [T][C]): what the comparison of a scaled call with the unscaled one allows on top of
    TOL_RATES (scale + |value|).  m_scaled [T][n] the site values at the scaled sites, blen [T][N-1][2], weights [C].
    2^-1075 is below the smallest subnormal, so the unit is written as 2^-55 / (m 2^1020)."""
    per_m = (2.0 ** -55 / (np.asarray(m_scaled) * 2.0 ** 1020)).sum(axis=1)           # sum_s 2^-1075 / m_s  [T]
    w = np.asarray(weights, dtype=np.float64)
    ex_w = np.broadcast_to((K_W * per_m)[:, None], (per_m.size, w.size))
    ex_r = K_R * per_m[:, None] * np.asarray(blen).sum(axis=(1, 2))[:, None] * w[None, :]
    return ex_r, ex_w


def close_with_excess(name, got, ref, scale, excess):
    """|got - ref| <= TOL_RATES (scale + |ref|) + excess, entry by entry; prints the worst ratio to that bound"""
    bound = TOL_RATES * (scale + np.abs(ref)) + excess
    diff = np.abs(got - ref)
    ratio = np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff == 0, 0.0, np.inf))
    print("%s: worst |difference| / (TOL_RATES (scale + |value|) + floor excess) = %.3g" % (name, np.nanmax(ratio)))
    assert np.isfinite(got).all(), name
    assert (ratio <= 1.0).all(), (name, float(np.nanmax(ratio)))
    return float(np.nanmax(ratio))


def one_site_below(X0, s=129):
    """the exponent of test_one_site_below_the_floor_spoils_its_tree_alone: with e the third smallest of X0[:, s] lands in
    [2^-1021, 2^-1020)"""
    order = np.argsort(X0[:, s])
    return int(np.frexp(X0[order[2], s])[1]) + 1020


def scale_one_site(g, e, s=129):
    gs = g.copy()
    gs[0, s], gs[1, s] = np.ldexp(g[0, s], -(e // 2)), np.ldexp(g[1, s], -(e - e // 2))
    return gs
