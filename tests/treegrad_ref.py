"""Restatement in plain NumPy of phylo_trees_grad's contract, independent of the library: one tree at a
time, loops over nodes, states and sides, arrays over the sites.  The branch matrices are INPUT (M [N-1][2][4][4] in the tree's
row order, M[i][side] the matrix of the branch above child[i][side]), so that whoever computes expm stays out of a comparison.

    x_v = (x_l . M_l) * (x_r . M_r)          L_s = prior . x_root[s]
    abar_root = prior;  g_l = abar_v * msg_r;  abar_l[k] = sum_j M_l[k][j] g_l[j]      (and l <-> r)
    L'_s(b) = sum_k x_child[k] sum_j M'_b[k][j] g_b[j],  M' = M Q,  M'' = M' Q
    grad = sum_s L'/L,  curv = sum_s (L''/L - (L'/L)^2),  scale = sum_s |L'/L|

The range: a tree with a site factor L_s below FLOOR = 2^-1020, or not finite, gets NaN in every derivative entry (1 / L_s is
no double below 2^-1024, and a subnormal L_s holds a handful of bits); its loglik is what it is.

`site_terms` is the same for ONE site over any number type (floats, mpmath's mpf): the high-precision yardstick of the tests."""
import numpy as np

FLOOR = 2.0 ** -1020     # the smallest site factor whose tree still gets derivatives


def dmat(M, Q):
    """M Q with the sum in ascending inner index, every product and sum rounded on its own (ptg_dmats' order)"""
    out = np.empty_like(M)
    for k in range(4):
        for j in range(4):
            out[..., k, j] = ((M[..., k, 0] * Q[0, j] + M[..., k, 1] * Q[1, j]) + M[..., k, 2] * Q[2, j]) + M[..., k, 3] * Q[3, j]
    return out


def fma(a, b, c):
    """round(a b + c) with ONE rounding, as the device's fma: the product exactly as p + e (Veltkamp's split, Dekker's product),
    p + c exactly as s + t (Knuth's sum), then s + (t + e).  Exact unless a b + c lies within 2^-106 of its size of a rounding
    boundary, or a value is near the ends of the double range (|a|, |b| < 1e300, |a b| > 1e-290).  Partials of alignments whose
    site factors stay above 1e-290 are inside; towards FLOOR they are not: there the error term e of the product underflows and
    this is an ordinary chain of rounded operations, within an ulp or so of the device's fma and no longer its bits.  Nothing
    is claimed bit for bit per site down there; the tolerance of the tests covers it (treegrad_cases.E_REF_FLOOR)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    p = a * b
    ah = a * 134217729.0
    ah = ah - (ah - a)
    al = a - ah
    bh = b * 134217729.0
    bh = bh - (bh - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    return s + (t + e)


def _row_times(x, M):
    """(x . M)[s][j], the fma chain of pt2_row_times"""
    out = np.empty_like(x)
    for j in range(4):
        out[:, j] = fma(x[:, 3], M[3, j], fma(x[:, 2], M[2, j], fma(x[:, 1], M[1, j], x[:, 0] * M[0, j])))
    return out


def _upward(child, M, prior, leaves):
    """the upward pass: every node's partial x [N + R] of [S][4], the messages [R][2][S][4] and the site factors L [S]"""
    N, S = leaves.shape[0], leaves.shape[1]
    R = N - 1
    x = [leaves[i] for i in range(N)] + [None] * R
    msg = np.empty((R, 2, S, 4))
    with np.errstate(all='ignore'):
        for i in range(R):
            for sd in range(2):
                msg[i, sd] = _row_times(x[child[i, sd]], M[i, sd])
            x[N + i] = msg[i, 0] * msg[i, 1]
        xr = x[N + R - 1]
        L = fma(prior[3], xr[:, 3], fma(prior[2], xr[:, 2], fma(prior[1], xr[:, 1], prior[0] * xr[:, 0])))     # pk_site_lik's chain
    return x, msg, L


def site_factors(child, M, prior, leaves):
    """L_s [S] of one tree: what the preconditions of the tests are read from"""
    return _upward(np.asarray(child), np.asarray(M, dtype=np.float64), np.asarray(prior, dtype=np.float64).reshape(4), leaves)[2]


def trees_site_factors(child, M, prior, leaves):
    return np.array([site_factors(c, m, prior, leaves) for c, m in zip(child, M)])


def tree_grad(child, M, Q, prior, leaves, want_sites=False):
    """child [N-1][2], M [N-1][2][4][4], leaves [N][S][4]  ->  loglik, grad, curv, scale (the last three [N-1][2]); with
    want_sites the site factors L [S] as a fifth"""
    child = np.asarray(child)
    N, S = leaves.shape[0], leaves.shape[1]
    R = N - 1
    M = np.asarray(M, dtype=np.float64)
    M1 = dmat(M, Q)
    M2 = dmat(M1, Q)
    prior = np.asarray(prior, dtype=np.float64).reshape(4)
    x, msg, L = _upward(child, M, prior, leaves)
    abar = [None] * (N + R)
    abar[N + R - 1] = np.broadcast_to(prior, (S, 4))
    grad, curv, scale = np.empty((R, 2)), np.empty((R, 2)), np.empty((R, 2))
    with np.errstate(all='ignore'):
        inv = 1.0 / L
        for i in range(R - 1, -1, -1):
            for sd in range(2):
                ch = child[i, sd]
                g = abar[N + i] * msg[i, 1 - sd]
                d1, d2 = np.zeros(S), np.zeros(S)
                for k in range(4):
                    t1 = ((M1[i, sd, k, 0] * g[:, 0] + M1[i, sd, k, 1] * g[:, 1]) + M1[i, sd, k, 2] * g[:, 2]) + M1[i, sd, k, 3] * g[:, 3]
                    t2 = ((M2[i, sd, k, 0] * g[:, 0] + M2[i, sd, k, 1] * g[:, 1]) + M2[i, sd, k, 2] * g[:, 2]) + M2[i, sd, k, 3] * g[:, 3]
                    d1 = d1 + x[ch][:, k] * t1
                    d2 = d2 + x[ch][:, k] * t2
                r1 = d1 * inv
                grad[i, sd] = np.sum(r1)
                scale[i, sd] = np.sum(np.abs(r1))
                curv[i, sd] = np.sum(d2 * inv - r1 * r1)
                if ch >= N:
                    a = np.empty((S, 4))
                    for k in range(4):
                        a[:, k] = ((M[i, sd, k, 0] * g[:, 0] + M[i, sd, k, 1] * g[:, 1]) + M[i, sd, k, 2] * g[:, 2]) + M[i, sd, k, 3] * g[:, 3]
                    abar[ch] = a
        loglik = float(np.sum(np.log(L)))
    if not (np.isfinite(loglik) and np.isfinite(L).all() and (L >= FLOOR).all()):
        grad[:], curv[:] = np.nan, np.nan
    return (loglik, grad, curv, scale, L) if want_sites else (loglik, grad, curv, scale)


def trees_grad(child, M, Q, prior, leaves, want_sites=False):
    """T trees: child [T][N-1][2], M [T][N-1][2][4][4]  ->  loglik [T], grad, curv, scale [T][N-1][2] (and L [T][S])"""
    res = [tree_grad(c, m, Q, prior, leaves, want_sites) for c, m in zip(child, M)]
    return tuple(np.array([r[k] for r in res]) for k in range(5 if want_sites else 4))


def site_terms(child, M, Q, prior, rows, zero):
    """One site over any number type: rows[i] the leaf's four values, M and Q nested lists of that type, `zero` its zero.
    Returns L and lists d1, d2 [N-1][2] of L' and L''."""
    N = len(rows)
    R = N - 1

    def mm(A, B):
        return [[sum((A[k][m] * B[m][j] for m in range(4)), zero) for j in range(4)] for k in range(4)]

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
    d1 = [[None, None] for _ in range(R)]
    d2 = [[None, None] for _ in range(R)]
    for i in range(R - 1, -1, -1):
        for sd in range(2):
            ch = child[i][sd]
            g = [abar[N + i][j] * msg[i][1 - sd][j] for j in range(4)]
            M1 = mm(M[i][sd], Q)
            M2 = mm(M1, Q)
            d1[i][sd] = sum((x[ch][k] * sum((M1[k][j] * g[j] for j in range(4)), zero) for k in range(4)), zero)
            d2[i][sd] = sum((x[ch][k] * sum((M2[k][j] * g[j] for j in range(4)), zero) for k in range(4)), zero)
            if ch >= N:
                abar[ch] = [sum((M[i][sd][k][j] * g[j] for j in range(4)), zero) for k in range(4)]
    return L, d1, d2
