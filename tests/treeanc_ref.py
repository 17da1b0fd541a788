"""Restatement in plain NumPy of phylo_trees_ancestral's contract, independent of the library: one tree at
a time, loops over nodes and states, arrays over the sites.  The branch matrices are INPUT, as in treegrad_ref.py, whose upward
pass (`_upward`, with its fma) this builds on.

    x_v = msg_l * msg_r            L_s = prior . x_root[s]          inv = 1 / L_s
    abar_root = prior;  g_l = abar_v * msg_r;  abar_l[k] = sum_j M_l[k][j] g_l[j]      (and l <-> r; section 13's recursion)
    post[v][s][j] = (abar_v[j] * x_v[j]) * inv                       three products, each rounded on its own; not renormalised
    state = the lowest j whose post is the largest of the four, NOSTATE if any is NaN;  pmax = post[state] or NaN

The range, per SITE: a site whose L_s lies below FLOOR = 2^-1020 or is not finite has NaN / NOSTATE in its own column at every
node; no other site sees it.

`site_terms` is the same for ONE site over any number type (floats, mpmath's mpf): the high-precision yardstick of the tests."""
import numpy as np

from treegrad_ref import FLOOR, _upward, fma  # noqa: F401  (fma: the chain inside _upward, re-exported for the tests)

NOSTATE = 255


def map_states(post):
    """state (uint8) and pmax of post [...][4] by the contract's rule, read from those very bits"""
    bad = np.isnan(post).any(axis=-1)
    best = np.zeros(post.shape[:-1], dtype=np.int64)
    pb = post[..., 0].copy()
    with np.errstate(invalid='ignore'):
        for j in range(1, 4):
            up = post[..., j] > pb                  # strictly larger: the lowest j among equals
            best[up] = j
            pb = np.where(up, post[..., j], pb)
    state = best.astype(np.uint8)
    state[bad] = NOSTATE
    return state, np.where(bad, np.nan, pb)


def tree_ancestral(child, M, prior, leaves):
    """child [N-1][2], M [N-1][2][4][4], leaves [N][S][4]  ->  loglik, post [N-1][S][4], state [N-1][S], pmax [N-1][S], L [S]"""
    child = np.asarray(child)
    N, S = leaves.shape[0], leaves.shape[1]
    R = N - 1
    M = np.asarray(M, dtype=np.float64)
    prior = np.asarray(prior, dtype=np.float64).reshape(4)
    x, msg, L = _upward(child, M, prior, leaves)
    abar = [None] * (N + R)
    abar[N + R - 1] = np.broadcast_to(prior, (S, 4))
    post = np.empty((R, S, 4))
    with np.errstate(all='ignore'):
        inv = np.where(np.isfinite(L) & (L >= FLOOR), 1.0 / L, np.nan)
        for i in range(R - 1, -1, -1):
            post[i] = (abar[N + i] * (msg[i, 0] * msg[i, 1])) * inv[:, None]
            for sd in range(2):
                ch = child[i, sd]
                if ch >= N:
                    g = abar[N + i] * msg[i, 1 - sd]
                    a = np.empty((S, 4))
                    for k in range(4):
                        a[:, k] = ((M[i, sd, k, 0] * g[:, 0] + M[i, sd, k, 1] * g[:, 1]) + M[i, sd, k, 2] * g[:, 2]) + M[i, sd, k, 3] * g[:, 3]
                    abar[ch] = a
        loglik = float(np.sum(np.log(L)))
    state, pmax = map_states(post)
    return loglik, post, state, pmax, L


def trees_ancestral(child, M, prior, leaves):
    """T trees: child [T][N-1][2], M [T][N-1][2][4][4]  ->  loglik [T], post [T][N-1][S][4], state, pmax [T][N-1][S], L [T][S]"""
    res = [tree_ancestral(c, m, prior, leaves) for c, m in zip(child, M)]
    return tuple(np.array([r[k] for r in res]) for k in range(5))


def site_terms(child, M, prior, rows, zero):
    """One site over any number type: rows[i] the leaf's four values, M nested lists of that type, `zero` its zero.
    Returns L and post [N-1][4] (divided by L, not renormalised)."""
    N = len(rows)
    R = N - 1
    x = list(rows) + [None] * R
    msg = [[None, None] for _ in range(R)]
    for i in range(R):
        for sd in range(2):
            xc = x[child[i][sd]]
            msg[i][sd] = [sum((xc[k] * M[i][sd][k][j] for k in range(4)), zero) for j in range(4)]
        x[N + i] = [msg[i][0][j] * msg[i][1][j] for j in range(4)]
    L = sum((prior[j] * x[N + R - 1][j] for j in range(4)), zero)
    abar = [None] * (N + R)
    abar[N + R - 1] = list(prior)
    post = [None] * R
    for i in range(R - 1, -1, -1):
        post[i] = [abar[N + i][j] * x[N + i][j] / L for j in range(4)]
        for sd in range(2):
            ch = child[i][sd]
            if ch >= N:
                g = [abar[N + i][j] * msg[i][1 - sd][j] for j in range(4)]
                abar[ch] = [sum((M[i][sd][k][j] * g[j] for j in range(4)), zero) for k in range(4)]
    return L, post
