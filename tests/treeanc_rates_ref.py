"""Restatement in plain NumPy of phylo_trees_ancestral_rates' contract, independent of the library: one
tree at a time, the categories a leading axis, arrays over the sites.  The branch matrices of every category are INPUT (M
[C][N-1][2][4][4], M[c][i][side] the matrix of the branch above child[i][side] at length rate[c] * blen[i][side]).  Built on
treegrad_ref's emulated fma (looked up at call time, so treegrad_edges_cases.hardware_fma reaches it), treegrad_rates_ref's upward
chain and section 13's downward recursion per category.

    per category c:  x_{v,c} = msg_l,c * msg_r,c;  f_c = prior . x_root,c (pk_site_lik's chain)
                     abar_root,c = prior;  g_l = abar_v * msg_r;  abar_l[k] = sum_j M_l[k][j] g_l[j]      (and l <-> r)
    m = w_0 f_0, then fma(w_c, f_c, m);   inv = 1 / m if m >= FLOOR and finite, else NaN
    acc_j = +0.0;  acc_j = acc_j + w_c * (abar_{v,c}[j] * (msg_l,c[j] * msg_r,c[j]))   c ascending;   post = acc_j * inv
    state, pmax = treeanc_ref.map_states(post)
    catpost_c = (w_c * f_c) * inv;    e = +0.0;  e = e + r_c * catpost_c   c ascending;   siterate = e

The range, per SITE: a site whose m lies below FLOOR = 2^-1020 or is not finite has NaN / NOSTATE in its own column of all five
outputs; no other site sees it.

`site_terms_rates` is the same for ONE site over any number type (floats, mpmath's mpf): the high-precision yardstick of the tests."""
import numpy as np

import rates_ref
import treegrad_rates_ref as RR
import treegrad_ref as TR
from treeanc_ref import NOSTATE, map_states  # noqa: F401
from treegrad_ref import FLOOR


def tree_ancestral_rates(child, M, prior, leaves, rates, weights, exact_mix=True):
    """child [N-1][2], M [C][N-1][2][4][4], leaves [N][S][4], rates and weights [C]  ->  a dict: 'loglik', 'post' [N-1][S][4],
    'state', 'pmax' [N-1][S], 'catpost' [C][S], 'siterate' [S], 'm' [S], 'f' [C][S].  exact_mix False: the mixing chain by
    treegrad_ref.fma over whole arrays instead of rates_ref.mix's exact fractions site by site"""
    child = np.asarray(child)
    N, S = leaves.shape[0], leaves.shape[1]
    R = N - 1
    M = np.asarray(M, dtype=np.float64)
    C = M.shape[0]
    prior = np.asarray(prior, dtype=np.float64).reshape(4)
    r, w = np.asarray(rates, dtype=np.float64).reshape(-1), np.asarray(weights, dtype=np.float64).reshape(-1)
    assert r.size == w.size == C
    x = [np.broadcast_to(leaves[i], (C, S, 4)) for i in range(N)] + [None] * R
    msg = [[None, None] for _ in range(R)]
    with np.errstate(all='ignore'):
        for i in range(R):
            for sd in range(2):
                msg[i][sd] = RR._row_times(x[child[i, sd]], M[:, i, sd])
            x[N + i] = msg[i][0] * msg[i][1]
        xr = x[N + R - 1]
        f = TR.fma(prior[3], xr[..., 3], TR.fma(prior[2], xr[..., 2], TR.fma(prior[1], xr[..., 1], prior[0] * xr[..., 0])))     # [C][S]
        if exact_mix and np.isfinite(f).all():
            m = rates_ref.mix(w, f)
        else:
            m = w[0] * f[0]
            for c in range(1, C):
                m = TR.fma(w[c], f[c], m)
        inv = np.where(np.isfinite(m) & (m >= FLOOR), 1.0 / m, np.nan)
        abar = [None] * (N + R)
        abar[N + R - 1] = np.broadcast_to(prior, (C, S, 4))
        post = np.empty((R, S, 4))
        for i in range(R - 1, -1, -1):
            q = abar[N + i] * (msg[i][0] * msg[i][1])       # [C][S][4]: two products
            acc = np.zeros((S, 4))
            for c in range(C):
                acc = acc + w[c] * q[c]
            post[i] = acc * inv[:, None]
            for sd in range(2):
                ch = child[i, sd]
                if ch >= N:
                    abar[ch] = RR._mat_times(M[:, i, sd], abar[N + i] * msg[i][1 - sd])
        catpost = (w[:, None] * f) * inv[None, :]
        e = np.zeros(S)
        for c in range(C):
            e = e + r[c] * catpost[c]
        loglik = float(np.sum(np.log(m)))
    state, pmax = map_states(post)
    return {'loglik': loglik, 'post': post, 'state': state, 'pmax': pmax, 'catpost': catpost, 'siterate': e, 'm': m, 'f': f}


def trees_ancestral_rates(child, M, prior, leaves, rates, weights, exact_mix=True):
    """T trees: child [T][N-1][2], M [T][C][N-1][2][4][4]; rates and weights [C] or [T][C]  ->  the dict of tree_ancestral_rates
    with a leading axis T"""
    rates, weights = np.asarray(rates, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    res = [tree_ancestral_rates(child[t], M[t], prior, leaves, rates[t] if rates.ndim == 2 else rates,
                                weights[t] if weights.ndim == 2 else weights, exact_mix) for t in range(len(child))]
    return {k: np.array([x[k] for x in res]) for k in res[0]}


def site_terms_rates(child, M, prior, rows, rates, weights, zero):
    """One site over any number type: rows[i] the leaf's four values, M [C] nested lists of that type, `zero` its zero.
    Returns m, post [N-1][4], catpost [C], siterate and f [C] -- the sums over the categories first, ONE division by m (a category
    with f_c = 0 is ordinary)."""
    C = len(rates)
    N = len(rows)
    R = N - 1
    num = [[zero] * 4 for _ in range(R)]
    f = []
    for c in range(C):
        x = list(rows) + [None] * R
        msg = [[None, None] for _ in range(R)]
        for i in range(R):
            for sd in range(2):
                xc = x[child[i][sd]]
                msg[i][sd] = [sum((xc[k] * M[c][i][sd][k][j] for k in range(4)), zero) for j in range(4)]
            x[N + i] = [msg[i][0][j] * msg[i][1][j] for j in range(4)]
        f.append(sum((prior[j] * x[N + R - 1][j] for j in range(4)), zero))
        abar = [None] * (N + R)
        abar[N + R - 1] = list(prior)
        for i in range(R - 1, -1, -1):
            for j in range(4):
                num[i][j] = num[i][j] + weights[c] * (abar[N + i][j] * x[N + i][j])
            for sd in range(2):
                ch = child[i][sd]
                if ch >= N:
                    g = [abar[N + i][j] * msg[i][1 - sd][j] for j in range(4)]
                    abar[ch] = [sum((M[c][i][sd][k][j] * g[j] for j in range(4)), zero) for k in range(4)]
    m = sum((weights[c] * f[c] for c in range(C)), zero)
    post = [[num[i][j] / m for j in range(4)] for i in range(R)]
    catpost = [weights[c] * f[c] / m for c in range(C)]
    siterate = sum((rates[c] * catpost[c] for c in range(C)), zero)
    return m, post, catpost, siterate, f
