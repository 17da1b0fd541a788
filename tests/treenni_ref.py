"""Restatement in plain NumPy of phylo_trees_nni's contract, independent of the library: one tree at a
time, loops over nodes and sides, arrays over the sites, the fma chains of the upward pass emulated by treegrad_ref.py.  The
branch matrices are INPUT (M [N-1][2][4][4] in the tree's row order), as in treegrad_ref.py.

    row i < N-2, v = N + i, parent p, sibling c, y = child[i][side], z = child[i][1 - side]:
        x_v' = msg(x_z, M_z) * msg(x_c, M_c);  x_p' = msg(x_v', M_v) * msg(x_y, M_y);  L'_s = chain(abar_p, x_p')
    row N-2, v = child[N-2][0] = (a, b), c = child[N-2][1] = (d, e), both internal, x = c's child on `side`, w its other:
        x_v' = msg(x_a) * msg(x_x);  x_c' = msg(x_w) * msg(x_b);  x_root' = msg(x_v', M_v) * msg(x_c', M_c);  L'_s = chain(prior, x_root')
    d_s = log(L'_s (1 / L_s)),  delta = sum_s d_s,  absd = sum_s |d_s|

Every subtree keeps the matrix of the branch above it.  NaN rule: treegrad_ref's (a site factor below FLOOR or not finite, or a
log-likelihood that is not finite: NaN in every entry); a move that does not exist is NaN.

`site_moves` is the same for ONE site over any number type (floats, mpmath's mpf): the high-precision yardstick of the tests."""
import numpy as np

import treegrad_ref as TR


def _chain(p, x):
    """pk_site_lik's chain with p [S][4] (or [4]) in the prior's place"""
    p = np.broadcast_to(p, x.shape)
    return TR.fma(p[:, 3], x[:, 3], TR.fma(p[:, 2], x[:, 2], TR.fma(p[:, 1], x[:, 1], p[:, 0] * x[:, 0])))


def tree_nni(child, M, prior, leaves, want_sites=False):
    """child [N-1][2], M [N-1][2][4][4], leaves [N][S][4]  ->  loglik, delta [N-1][2], absd [N-1][2] (sum_s |d_s|; with want_sites
    the site factors L [S] as a fourth)"""
    child = np.asarray(child)
    N, S = leaves.shape[0], leaves.shape[1]
    R = N - 1
    M = np.asarray(M, dtype=np.float64)
    prior = np.asarray(prior, dtype=np.float64).reshape(4)
    x, msg, L = TR._upward(child, M, prior, leaves)
    abar = [None] * (N + R)
    abar[N + R - 1] = np.broadcast_to(prior, (S, 4))
    delta, absd = np.full((R, 2), np.nan), np.full((R, 2), np.nan)

    def put(i, sd, Lp, inv):
        d = np.log(Lp * inv)
        delta[i, sd] = np.sum(d)
        absd[i, sd] = np.sum(np.abs(d))

    with np.errstate(all='ignore'):
        inv = 1.0 / L
        r = R - 1
        v, c = int(child[r, 0]) - N, int(child[r, 1]) - N
        if v >= 0 and c >= 0:
            for sd in range(2):
                xv = msg[v, 0] * msg[c, sd]
                xc = msg[c, 1 - sd] * msg[v, 1]
                put(r, sd, _chain(prior, TR._row_times(xv, M[r, 0]) * TR._row_times(xc, M[r, 1])), inv)
        for p in range(R - 1, -1, -1):
            for sdv in range(2):
                ch = int(child[p, sdv])
                if ch < N:
                    continue
                i = ch - N
                for sd in range(2):
                    xv = msg[i, 1 - sd] * msg[p, 1 - sdv]
                    xp = TR._row_times(xv, M[p, sdv]) * msg[i, sd]
                    put(i, sd, _chain(abar[N + p], xp), inv)
                g = abar[N + p] * msg[p, 1 - sdv]
                a = np.empty((S, 4))
                for k in range(4):
                    a[:, k] = ((M[p, sdv, k, 0] * g[:, 0] + M[p, sdv, k, 1] * g[:, 1]) + M[p, sdv, k, 2] * g[:, 2]) + M[p, sdv, k, 3] * g[:, 3]
                abar[ch] = a
        loglik = float(np.sum(np.log(L)))
    if not (np.isfinite(loglik) and np.isfinite(L).all() and (L >= TR.FLOOR).all()):
        delta[:] = np.nan
    return (loglik, delta, absd, L) if want_sites else (loglik, delta, absd)


def trees_nni(child, M, prior, leaves):
    """T trees: child [T][N-1][2], M [T][N-1][2][4][4]  ->  loglik [T], delta, absd [T][N-1][2]"""
    res = [tree_nni(c, m, prior, leaves) for c, m in zip(child, M)]
    return tuple(np.array([r[k] for r in res]) for k in range(3))


def tree_loglik_sites(child, M, prior, leaves):
    """loglik and sum_s |log L_s| of one tree by the restated upward pass"""
    L = TR.site_factors(child, M, prior, leaves)
    with np.errstate(all='ignore'):
        lg = np.log(L)
    return float(np.sum(lg)), float(np.sum(np.abs(lg)))


def site_moves(child, M, prior, rows, zero):
    """One site over any number type: rows[i] the leaf's four values, M nested lists of that type, `zero` its zero.  Returns L and
    a dict {(row, side): L'} over the moves that exist."""
    N = len(rows)
    R = N - 1

    def times(xc, m):
        return [sum((xc[k] * m[k][j] for k in range(4)), zero) for j in range(4)]

    def dot(p, xx):
        return sum((p[j] * xx[j] for j in range(4)), zero)

    x = list(rows) + [None] * R
    msg = [[None, None] for _ in range(R)]
    for i in range(R):
        for sd in range(2):
            msg[i][sd] = times(x[child[i][sd]], M[i][sd])
        x[N + i] = [msg[i][0][j] * msg[i][1][j] for j in range(4)]
    L = dot(prior, x[N + R - 1])
    abar = [None] * (N + R)
    abar[N + R - 1] = list(prior)
    out = {}
    r = R - 1
    v, c = child[r][0] - N, child[r][1] - N
    if v >= 0 and c >= 0:
        for sd in range(2):
            xv = [msg[v][0][j] * msg[c][sd][j] for j in range(4)]
            xc = [msg[c][1 - sd][j] * msg[v][1][j] for j in range(4)]
            tv, tc = times(xv, M[r][0]), times(xc, M[r][1])
            out[(r, sd)] = dot(prior, [tv[j] * tc[j] for j in range(4)])
    for p in range(R - 1, -1, -1):
        for sdv in range(2):
            ch = child[p][sdv]
            if ch < N:
                continue
            i = ch - N
            for sd in range(2):
                xv = [msg[i][1 - sd][j] * msg[p][1 - sdv][j] for j in range(4)]
                t = times(xv, M[p][sdv])
                out[(i, sd)] = dot(abar[N + p], [t[j] * msg[i][sd][j] for j in range(4)])
            g = [abar[N + p][j] * msg[p][1 - sdv][j] for j in range(4)]
            abar[ch] = [sum((M[p][sdv][k][j] * g[j] for j in range(4)), zero) for k in range(4)]
    return L, out
