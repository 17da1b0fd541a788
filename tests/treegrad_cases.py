"""Shared inputs of the branch-length gradient tests: alignments simulated along a tree, and E_REF, the
worst error of the NumPy restatement (treegrad_ref.py) against the same formulas at 50 digits, which sets the device tolerance."""
import numpy as np
from scipy.linalg import expm

# Measured by test_treegrad_cpu.py::test_reference_against_mpmath (N = 5, S = 8, gaps; grad and curv, GTR and JC69): the worst
# |reference - 50-digit value| / ((scale + |value|) 2^-53) is 8.59; the test asserts that it stays at or below E_REF.
E_REF = 8.6
# Measured by test_trees_edges_cpu.py::test_reference_against_mpmath_at_the_floor (the same 40 trees, every site factor scaled into
# [2^-1020, 2^-1000] through two leaves): 8.59 in the same units -- the floor costs the restatement nothing, so 2^-1020, the bound
# the sweep's reverse pass states, is the bound below which phylo_trees_grad gives NaN, and TOL holds down to it.
E_REF_FLOOR = 8.6
TOL = 8 * E_REF * 2.0 ** -53         # device against reference: |difference| <= TOL (scale + |value|)


def branch_matrices(Q, blen):
    """expm(Q t) of every length of blen [...]: [...][4][4], by scipy"""
    blen = np.asarray(blen, dtype=np.float64)
    return np.array([expm(Q * t) for t in blen.reshape(-1)]).reshape(blen.shape + (4, 4))


def simulate(child, blen, Q, pi, S, rng):
    """an alignment [N][S][4] of indicator rows evolved down the tree (rows as trees_cases gives them) from a root drawn from pi"""
    R = child.shape[0]
    N = R + 1
    st = np.empty((N + R, S), dtype=np.int64)
    st[N + R - 1] = rng.choice(4, size=S, p=pi)
    for i in range(R - 1, -1, -1):
        for sd in range(2):
            cum = np.cumsum(expm(Q * blen[i, sd])[st[N + i]], axis=1)
            st[child[i, sd]] = np.minimum((rng.random(S)[:, None] > cum).sum(axis=1), 3)
    g = np.zeros((N, S, 4))
    for i in range(N):
        g[i, np.arange(S), st[i]] = 1.0
    return g
