"""Restatement in plain NumPy of phylo_trees_grad_rates' contract, independent of the library, over
treegrad_ref's dmat and fma, its upward pass with the categories as a leading axis, and rates_ref's mixing chain.  One tree at a time; the branch matrices of every category
are INPUT (M [C][N-1][2][4][4], M[c][i][side] the matrix of the branch above child[i][side] at length rate[c] * blen[i][side]).

    per category c:  f_c[s], D1_c[b][s] = L', D2_c[b][s] = L'' of section 13 inside the category (treegrad_ref's recursion)
    m = w_0 f_0, then fma(w_c, f_c, m);  u_c = w_c r_c, v_c = u_c r_c
    a1 = sum_c u_c D1_c, a2 = sum_c v_c D2_c   (c ascending, from +0.0)
    grad = sum_s a1 / m,  curv = sum_s (a2 / m - (a1 / m)^2),  scale = sum_s |a1 / m|
    drate_c = sum_s sum_b (blen_b w_c) D1_c[b] / m,  its scale the same sum of absolute values
    dweight_c = sum_s f_c / m, which is its own scale

The NaN rule is section 13's on m: a tree with an m below FLOOR, or not finite, or whose loglik is not finite, gets NaN in all four."""
import numpy as np

import rates_ref
import treegrad_ref as TR
from treegrad_ref import FLOOR


def _row_times(x, M):
    """(x . M)[c][s][j] for x [C][S][4] and M [C][4][4]: the fma chain of pt2_row_times (treegrad_ref._row_times with a leading
    category axis, so that a tree's C upward passes are one pass over arrays C times as long)"""
    out = np.empty_like(x)
    for j in range(4):
        m = M[:, :, j, None]
        out[..., j] = TR.fma(x[..., 3], m[:, 3], TR.fma(x[..., 2], m[:, 2], TR.fma(x[..., 1], m[:, 1], x[..., 0] * m[:, 0])))
    return out


def _mat_times(M, g):
    """sum_j M[c][k][j] g[c][s][j] for every k, j ascending, every product and sum rounded on its own: [C][S][4]"""
    out = np.empty_like(g)
    for k in range(4):
        m = M[:, k, :, None]
        out[..., k] = ((m[:, 0] * g[..., 0] + m[:, 1] * g[..., 1]) + m[:, 2] * g[..., 2]) + m[:, 3] * g[..., 3]
    return out


def category_terms(child, M, Q, prior, leaves):
    """every category of one tree, M [C][N-1][2][4][4]: f [C][S], D1 and D2 [C][N-1][2][S] -- treegrad_ref's upward pass
    (pk_site_lik's chain at the root) and tree_grad's downward pass with the site terms kept, the categories a leading axis"""
    child = np.asarray(child)
    N, S = leaves.shape[0], leaves.shape[1]
    R = N - 1
    M = np.asarray(M, dtype=np.float64)
    C = M.shape[0]
    M1 = TR.dmat(M, Q)
    M2 = TR.dmat(M1, Q)
    x = [np.broadcast_to(leaves[i], (C, S, 4)) for i in range(N)] + [None] * R
    msg = [[None, None] for _ in range(R)]
    D1, D2 = np.empty((C, R, 2, S)), np.empty((C, R, 2, S))
    with np.errstate(all='ignore'):
        for i in range(R):
            for sd in range(2):
                msg[i][sd] = _row_times(x[child[i, sd]], M[:, i, sd])
            x[N + i] = msg[i][0] * msg[i][1]
        xr = x[N + R - 1]
        L = TR.fma(prior[3], xr[..., 3], TR.fma(prior[2], xr[..., 2], TR.fma(prior[1], xr[..., 1], prior[0] * xr[..., 0])))
        abar = [None] * (N + R)
        abar[N + R - 1] = np.broadcast_to(prior, (C, S, 4))
        for i in range(R - 1, -1, -1):
            for sd in range(2):
                ch = child[i, sd]
                g = abar[N + i] * msg[i][1 - sd]
                t1, t2 = _mat_times(M1[:, i, sd], g), _mat_times(M2[:, i, sd], g)
                xc = x[ch]
                D1[:, i, sd] = ((xc[..., 0] * t1[..., 0] + xc[..., 1] * t1[..., 1]) + xc[..., 2] * t1[..., 2]) + xc[..., 3] * t1[..., 3]   # ptg_xDg
                D2[:, i, sd] = ((xc[..., 0] * t2[..., 0] + xc[..., 1] * t2[..., 1]) + xc[..., 2] * t2[..., 2]) + xc[..., 3] * t2[..., 3]
                if ch >= N:
                    abar[ch] = _mat_times(M[:, i, sd], g)
    return L, D1, D2


def tree_grad_rates(child, M, Q, prior, leaves, blen, rates, weights, exact_mix=True):
    """child [N-1][2], M [C][N-1][2][4][4], blen [N-1][2] (the GIVEN lengths), rates and weights [C]  ->  a dict: 'loglik',
    'grad', 'curv', 'scale' [N-1][2], 'drate', 'drate_scale', 'dweight' [C], 'm' [S], 'f' [C][S].  exact_mix False: the mixing chain by treegrad_ref.fma over whole
    arrays instead of rates_ref.mix's exact fractions site by site (the same bits inside fma's range; for the optimiser's many calls)"""
    prior = np.asarray(prior, dtype=np.float64).reshape(4)
    blen = np.asarray(blen, dtype=np.float64)
    r, w = np.asarray(rates, dtype=np.float64).reshape(-1), np.asarray(weights, dtype=np.float64).reshape(-1)
    C = r.size
    R, S = blen.shape[0], leaves.shape[1]
    f, D1, D2 = category_terms(child, M, Q, prior, leaves)
    with np.errstate(all='ignore'):
        if exact_mix and np.isfinite(f).all():
            m = rates_ref.mix(w, f)
        else:
            m = w[0] * f[0]
            for c in range(1, C):
                m = TR.fma(w[c], f[c], m)
        inv = 1.0 / m
        a1, a2 = np.zeros((R, 2, S)), np.zeros((R, 2, S))
        drate, drate_scale, dweight = np.empty(C), np.empty(C), np.empty(C)
        for c in range(C):
            u = w[c] * r[c]
            v = u * r[c]
            a1 = a1 + u * D1[c]
            a2 = a2 + v * D2[c]
            part = ((blen * w[c])[:, :, None] * D1[c]) * inv
            drate[c] = part.sum()
            drate_scale[c] = np.abs(part).sum()
            dweight[c] = (f[c] * inv).sum()
        r1 = a1 * inv
        grad = r1.sum(axis=2)
        scale = np.abs(r1).sum(axis=2)
        curv = (a2 * inv - r1 * r1).sum(axis=2)
        loglik = float(np.sum(np.log(m)))
    if not (np.isfinite(loglik) and np.isfinite(m).all() and (m >= FLOOR).all()):
        grad, curv = np.full((R, 2), np.nan), np.full((R, 2), np.nan)
        drate, dweight = np.full(C, np.nan), np.full(C, np.nan)
    return {'loglik': loglik, 'grad': grad, 'curv': curv, 'scale': scale, 'drate': drate, 'drate_scale': drate_scale, 'dweight': dweight,
            'm': m, 'f': f}


def trees_grad_rates(child, M, Q, prior, leaves, blen, rates, weights):
    """T trees: child [T][N-1][2], M [T][C][N-1][2][4][4], blen [T][N-1][2]; rates and weights [C] or [T][C]  ->  the dict of
    tree_grad_rates with a leading axis T"""
    rates, weights = np.asarray(rates, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    T = len(child)
    res = [tree_grad_rates(child[t], M[t], Q, prior, leaves, blen[t], rates[t] if rates.ndim == 2 else rates,
                           weights[t] if weights.ndim == 2 else weights) for t in range(T)]
    return {k: np.array([r[k] for r in res]) for k in res[0]}


def site_terms_rates(child, M, Q, prior, rows, blen, rates, weights, zero):
    """One site over any number type (floats, mpmath's mpf), by treegrad_ref.site_terms per category: M [C] nested lists.
    Returns m, a1, a2 [N-1][2], the drate terms [C] (sum over the branches of blen_b w D1) and f [C]."""
    C = len(rates)
    R = len(child)
    per = [TR.site_terms(child, M[c], Q, prior, rows, zero) for c in range(C)]
    m = sum((weights[c] * per[c][0] for c in range(C)), zero)
    a1 = [[sum((weights[c] * rates[c] * per[c][1][i][sd] for c in range(C)), zero) for sd in range(2)] for i in range(R)]
    a2 = [[sum((weights[c] * rates[c] * rates[c] * per[c][2][i][sd] for c in range(C)), zero) for sd in range(2)] for i in range(R)]
    dr = [sum((blen[i][sd] * weights[c] * per[c][1][i][sd] for i in range(R) for sd in range(2)), zero) for c in range(C)]
    return m, a1, a2, dr, [per[c][0] for c in range(C)]
