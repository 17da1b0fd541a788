"""Restatement in plain NumPy of phylo_trees_grad_model's contract, independent of the library.  The
branch matrices M are INPUT, as in treegrad_ref.py (whoever computes expm stays out of a comparison); the direction matrices
D_{p,b} = L(Q t_b, E_p t_b) are made HERE, by pg_expm4_frechet restated term by term (`frechet`): the 1-norm and the scaling by
a power of two, the number of terms from theta, pm_mm4's fma chains (treegrad_ref.fma emulates the device's fma), the running
sums, the squarings.

    l_{p,b}[s] = (sum_k x_child[k] sum_j D_{p,b}[k][j] g_b[j]) (1 / L_s)         (ptg_xDg's order; x, g, L of treegrad_ref.py)
    dtheta[p]  = sum_s sum_b l_{p,b}[s]          dprior[j] = sum_s x_root[s][j] (1 / L_s)

in the device's order of summation: a site s of a tile of `tile` sites sits in lane (s - s0) % 64 of step ((s - s0) // 64) % 2 of
strip (s - s0) // 128; a lane adds, from +0.0, per strip, per operation (last to first) and side (left, right) the sum over its
two steps (ascending, from +0.0; a step past the end adds +0.0) -- for dprior each step's term on its own --; the 64 lanes go
through the adjacent-pair tree; the tiles are added left to right.  `order` is the schedule's order of the rows (what the device walks); without it the rows' own order, which
is a schedule too -- the sums then differ from the device's in the order over the branches, inside the tolerance.

TOL_MODEL: see E_REF_MODEL below.  `site_terms_model` is the same for ONE site over any number type (mpmath's mpf)."""
import numpy as np

import treegrad_ref as TR
from treegrad_ref import FLOOR, fma

# Measured by test_treegrad_model_cpu.py::test_reference_against_mpmath (N = 5, S = 8, gaps; 20 trees under a GTR-like Q and under
# JC69; the 12 softmax directions, Q itself and one random direction; dtheta and dprior): the worst |reference - 50-digit value|
# in units of (scale + |value|) 2^-53 is 2.634 (dtheta: 2.634, dprior: 1.273); the test asserts that it stays at or below E_REF_MODEL.
E_REF_MODEL = 2.7
TOL_MODEL = 8 * E_REF_MODEL * 2.0 ** -53      # device against reference: |difference| <= TOL_MODEL (scale + |value|)

JC_Q = np.full((4, 4), 0.25) - np.eye(4)       # the generator jc69_closed_form implies: 1/4, diagonal -3/4


def mm4(a, b):
    """pm_mm4 over stacks [n][4][4]: c[i][j] = a[i][0] b[0][j], then fma(a[i][m], b[m][j], .) for m = 1, 2, 3"""
    acc = a[:, :, 0, None] * b[:, None, 0, :]
    for m in range(1, 4):
        acc = fma(a[:, :, m, None], b[:, None, m, :], acc)
    return acc


def frechet(A0, E0):
    """pg_expm4_frechet over stacks A0, E0 [n][4][4] -> L [n][4][4].  Matrices that share (squarings, terms) run together."""
    A0, E0 = np.asarray(A0, dtype=np.float64), np.asarray(E0, dtype=np.float64)
    n = A0.shape[0]
    ab = np.abs(A0)
    cs = np.zeros((n, 4))
    for i in range(4):
        cs = cs + ab[:, i, :]                               # column sums, rows ascending from 0.0
    norm = np.zeros(n)
    for j in range(4):
        norm = np.where(cs[:, j] > norm, cs[:, j], norm)
    s = np.zeros(n, dtype=np.int64)
    lim = np.full(n, 0.5)
    for _ in range(60):
        more = norm > lim
        if not more.any():
            break
        lim = np.where(more, lim * 2.0, lim)
        s = s + more
    sc = np.ldexp(1.0, -s)
    theta = norm * sc
    nterms = np.where(theta <= 0.01, 8, np.where(theta <= 0.05, 10, np.where(theta <= 0.15, 13, np.where(theta <= 0.3, 15, 18))))
    out = np.empty((n, 4, 4))
    eye = np.eye(4)
    for key in sorted(set(zip(s.tolist(), nterms.tolist()))):
        sel = np.nonzero((s == key[0]) & (nterms == key[1]))[0]
        A, E = A0[sel] * sc[sel, None, None], E0[sel] * sc[sel, None, None]
        X = np.broadcast_to(eye, A.shape).copy()
        D = np.zeros(A.shape)
        SX, SD = X.copy(), D.copy()
        for k in range(1, key[1] + 1):
            inv = 1.0 / k                                   # correctly rounded, as the device's table
            D = (mm4(X, E) + mm4(D, A)) * inv
            X = mm4(X, A) * inv
            SX = SX + X
            SD = SD + D
        for _ in range(key[0]):
            SD = mm4(SX, SD) + mm4(SD, SX)
            SX = mm4(SX, SX)
        out[sel] = SD
    return out


def direction_matrices(Q, dirs, blen, jc=False):
    """D [...][P][4][4] for blen [...]: A = Q_eff t and E = dirs[p] t, one multiply per entry, then frechet"""
    Qe = JC_Q if jc else np.asarray(Q, dtype=np.float64)
    dirs = np.asarray(dirs, dtype=np.float64)
    blen = np.asarray(blen, dtype=np.float64)
    t = blen.reshape(-1)
    P = dirs.shape[0]
    A = np.repeat((Qe[None] * t[:, None, None])[:, None], P, axis=1).reshape(-1, 4, 4)
    E = (dirs[None] * t[:, None, None, None]).reshape(-1, 4, 4)
    return frechet(A, E).reshape(blen.shape + (P, 4, 4))


def wave_tree_sum(v):
    """pk_wave_tree_sum: 64 values by the adjacent-pair tree"""
    v = np.asarray(v, dtype=np.float64)
    while v.shape[0] > 1:
        v = v[0::2] + v[1::2]
    return float(v[0])


def _lane_sum(terms, tile, pair=True):
    """terms [n_ops][S] in the order the device walks them -> the device's sum: per tile, per lane over strips, operations and the
    two steps, the wave tree, the tiles left to right.  pair (dtheta): the two steps' terms are added to one another from +0.0
    and that sum goes into the lane's accumulator; not pair (dprior): each step's term goes into the accumulator on its own"""
    n_ops, S = terms.shape
    total = None
    for s0 in range(0, S, tile):
        s1 = min(s0 + tile, S)
        acc = np.zeros(64)
        for base in range(s0, s1, 128):
            pad = np.zeros((n_ops, 128))
            m = min(128, s1 - base)
            pad[:, :m] = terms[:, base:base + m]
            for k in range(n_ops):
                if pair:
                    acc = acc + ((0.0 + pad[k, :64]) + pad[k, 64:])
                else:
                    acc = (acc + pad[k, :64]) + pad[k, 64:]
        t = wave_tree_sum(acc)
        total = t if total is None else total + t
    return total


def tree_grad_model(child, M, D, prior, leaves, tile=None, order=None):
    """child [N-1][2], M [N-1][2][4][4], D [N-1][2][P][4][4] (rows in the tree's order), leaves [N][S][4]  ->  loglik, dtheta [P],
    dprior [4], scale_theta [P] = sum_s sum_b |l_{p,b}[s]|, scale_prior [4] = sum_s x_root[j] / L_s"""
    child = np.asarray(child)
    N, S = leaves.shape[0], leaves.shape[1]
    R = N - 1
    P = D.shape[2]
    tile = S if tile is None else tile
    order = list(range(R)) if order is None else list(order)
    prior = np.asarray(prior, dtype=np.float64).reshape(4)
    x, msg, L = TR._upward(child, np.asarray(M, dtype=np.float64), prior, leaves)
    abar = [None] * (N + R)
    abar[N + R - 1] = np.broadcast_to(prior, (S, 4))
    terms = np.empty((P, R, 2, S))
    with np.errstate(all='ignore'):
        inv = 1.0 / L
        for i in range(R - 1, -1, -1):
            for sd in range(2):
                ch = child[i, sd]
                g = abar[N + i] * msg[i, 1 - sd]
                for p in range(P):
                    Dm = D[i, sd, p]
                    d = np.zeros(S)
                    first = True
                    for k in range(4):
                        t = ((Dm[k, 0] * g[:, 0] + Dm[k, 1] * g[:, 1]) + Dm[k, 2] * g[:, 2]) + Dm[k, 3] * g[:, 3]
                        d = x[ch][:, k] * t if first else d + x[ch][:, k] * t
                        first = False
                    terms[p, i, sd] = d * inv
                if ch >= N:
                    a = np.empty((S, 4))
                    for k in range(4):
                        a[:, k] = ((M[i, sd, k, 0] * g[:, 0] + M[i, sd, k, 1] * g[:, 1]) + M[i, sd, k, 2] * g[:, 2]) + M[i, sd, k, 3] * g[:, 3]
                    abar[ch] = a
        walk = [(i, sd) for i in reversed(order) for sd in range(2)]          # operations last to first, left then right
        dtheta = np.array([_lane_sum(np.array([terms[p, i, sd] for i, sd in walk]), tile) for p in range(P)])
        scale_theta = np.abs(terms).sum(axis=(1, 2, 3))
        xr = x[N + R - 1]
        pt = xr * inv[:, None]
        dprior = np.array([_lane_sum(pt[None, :, j], tile, pair=False) for j in range(4)])
        scale_prior = np.abs(pt).sum(axis=0)
        loglik = float(np.sum(np.log(L)))
    if not (np.isfinite(loglik) and np.isfinite(L).all() and (L >= FLOOR).all()):
        dtheta[:], dprior[:] = np.nan, np.nan
    return loglik, dtheta, dprior, scale_theta, scale_prior


def trees_grad_model(child, M, D, prior, leaves, tile=None):
    """T trees  ->  loglik [T], dtheta [T][P], dprior [T][4], scale_theta [T][P], scale_prior [T][4]"""
    res = [tree_grad_model(c, m, d, prior, leaves, tile) for c, m, d in zip(child, M, D)]
    return tuple(np.array([r[k] for r in res]) for k in range(5))


def site_terms_model(child, M, D, prior, rows, zero):
    """One site over any number type: rows[i] the leaf's four values, M [N-1][2] and D [N-1][2][P] nested lists of that type.
    Returns L, the list [P] of sum_b x_child . D_{p,b} . g_b, the same of absolute values per branch, and x_root [4]."""
    N = len(rows)
    R = N - 1
    P = len(D[0][0])
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
    tot = [zero] * P
    tot_abs = [zero] * P
    for i in range(R - 1, -1, -1):
        for sd in range(2):
            ch = child[i][sd]
            g = [abar[N + i][j] * msg[i][1 - sd][j] for j in range(4)]
            for p in range(P):
                v = sum((x[ch][k] * sum((D[i][sd][p][k][j] * g[j] for j in range(4)), zero) for k in range(4)), zero)
                tot[p] = tot[p] + v
                tot_abs[p] = tot_abs[p] + abs(v)
            if ch >= N:
                abar[ch] = [sum((M[i][sd][k][j] * g[j] for j in range(4)), zero) for k in range(4)]
    return L, tot, tot_abs, x[N + R - 1]
