"""Restatement in plain NumPy of phylo_trees_nni_rates' contract, independent of the library, over
treenni_ref.py's formulas, treegrad_ref.py's upward pass and fma, and rates_ref.py's mixing chain.  One tree at a time; the branch
matrices of every category are INPUT (M [C][N-1][2][4][4], M[c][i][side] the matrix at length rate[c] * blen[i][side]).

    per category c: f_c[s] the tree's factor and f'_c[move][s] every neighbour's, section 14's formulas under M[c]
    m = w_0 f_0, then fma(w_c, f_c, m);  m' = w_0 f'_0, then fma(w_c, f'_c, m')       (rates_ref.mix)
    d_s = log(m'_s (1 / m_s)),  delta = sum_s d_s,  absd = sum_s |d_s|

NaN rule: section 13b's on m (an m below FLOOR or not finite, or a log-likelihood that is not finite: NaN in every entry); a move
that does not exist is NaN.  `site_moves_rates` is the same for ONE site over any number type: the high-precision yardstick."""
import numpy as np

import rates_ref
import treegrad_ref as TR
import treenni_ref as NR
from treegrad_ref import FLOOR


def category_factors(child, M, prior, leaves):
    """one category of one tree, M [N-1][2][4][4]: L [S] and {(row, side): L' [S]} over the moves that exist -- treenni_ref.tree_nni's
    formulas with the site factors kept"""
    child = np.asarray(child)
    N, S = leaves.shape[0], leaves.shape[1]
    R = N - 1
    x, msg, L = TR._upward(child, M, prior, leaves)
    abar = [None] * (N + R)
    abar[N + R - 1] = np.broadcast_to(prior, (S, 4))
    out = {}
    r = R - 1
    v, c = int(child[r, 0]) - N, int(child[r, 1]) - N
    if v >= 0 and c >= 0:
        for sd in range(2):
            xv = msg[v, 0] * msg[c, sd]
            xc = msg[c, 1 - sd] * msg[v, 1]
            out[(r, sd)] = NR._chain(prior, TR._row_times(xv, M[r, 0]) * TR._row_times(xc, M[r, 1]))
    for p in range(R - 1, -1, -1):
        for sdv in range(2):
            ch = int(child[p, sdv])
            if ch < N:
                continue
            i = ch - N
            for sd in range(2):
                xv = msg[i, 1 - sd] * msg[p, 1 - sdv]
                xp = TR._row_times(xv, M[p, sdv]) * msg[i, sd]
                out[(i, sd)] = NR._chain(abar[N + p], xp)
            g = abar[N + p] * msg[p, 1 - sdv]
            a = np.empty((S, 4))
            for k in range(4):
                a[:, k] = ((M[p, sdv, k, 0] * g[:, 0] + M[p, sdv, k, 1] * g[:, 1]) + M[p, sdv, k, 2] * g[:, 2]) + M[p, sdv, k, 3] * g[:, 3]
            abar[ch] = a
    return L, out


def _mix(w, f, exact):
    if exact and np.isfinite(f).all():
        return rates_ref.mix(w, f)
    m = w[0] * f[0]
    for c in range(1, len(w)):
        m = TR.fma(w[c], f[c], m)
    return m


def tree_nni_rates(child, M, prior, leaves, rates, weights, exact_mix=True, want_sites=False):
    """child [N-1][2], M [C][N-1][2][4][4], leaves [N][S][4], weights [C] (rates is not read: the matrices carry it)  ->  loglik,
    delta [N-1][2], absd [N-1][2] (with want_sites m [S] as a fourth).  exact_mix False: the mixing chain by treegrad_ref.fma over
    whole arrays instead of exact fractions site by site (the same bits inside fma's range; for the search's many calls)"""
    M = np.asarray(M, dtype=np.float64)
    prior = np.asarray(prior, dtype=np.float64).reshape(4)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    C = w.size
    assert M.shape[0] == C
    R = leaves.shape[0] - 1
    delta, absd = np.full((R, 2), np.nan), np.full((R, 2), np.nan)
    with np.errstate(all='ignore'):
        per = [category_factors(child, M[c], prior, leaves) for c in range(C)]
        m = _mix(w, np.array([p[0] for p in per]), exact_mix)
        inv = 1.0 / m
        for key in per[0][1]:
            mp = _mix(w, np.array([p[1][key] for p in per]), exact_mix)
            d = np.log(mp * inv)
            delta[key] = np.sum(d)
            absd[key] = np.sum(np.abs(d))
        loglik = float(np.sum(np.log(m)))
    if not (np.isfinite(loglik) and np.isfinite(m).all() and (m >= FLOOR).all()):
        delta[:] = np.nan
    return (loglik, delta, absd, m) if want_sites else (loglik, delta, absd)


def trees_nni_rates(child, M, prior, leaves, rates, weights, exact_mix=True):
    """T trees: child [T][N-1][2], M [T][C][N-1][2][4][4]; rates and weights [C] or [T][C]  ->  loglik [T], delta, absd [T][N-1][2]"""
    rates, weights = np.asarray(rates, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    res = [tree_nni_rates(child[t], M[t], prior, leaves, rates[t] if rates.ndim == 2 else rates,
                          weights[t] if weights.ndim == 2 else weights, exact_mix) for t in range(len(child))]
    return tuple(np.array([r[k] for r in res]) for k in range(3))


def tree_site_values(child, M, prior, leaves, weights):
    """m [S] of one tree by the restated upward pass of every category and the mixing chain"""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    with np.errstate(all='ignore'):
        f = np.array([TR.site_factors(child, M[c], prior, leaves) for c in range(w.size)])
        return _mix(w, f, True)


def tree_loglik_sites(child, M, prior, leaves, weights):
    """mixture loglik and sum_s |log m_s| of one tree"""
    with np.errstate(all='ignore'):
        lg = np.log(tree_site_values(child, M, prior, leaves, weights))
    return float(np.sum(lg)), float(np.sum(np.abs(lg)))


def site_moves_rates(child, M, prior, rows, weights, zero):
    """One site over any number type, by treenni_ref.site_moves per category: M [C] nested lists, weights [C] of that type.
    Returns m and a dict {(row, side): m'} over the moves that exist."""
    C = len(weights)
    per = [NR.site_moves(child, M[c], prior, rows, zero) for c in range(C)]
    m = sum((weights[c] * per[c][0] for c in range(C)), zero)
    return m, {key: sum((weights[c] * per[c][1][key] for c in range(C)), zero) for key in per[0][1]}
