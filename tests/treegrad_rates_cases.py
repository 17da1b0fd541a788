"""Shared inputs of the tests of phylo_trees_grad_rates: E_REF_RATES, the worst error of the NumPy
restatement (treegrad_rates_ref.py) against the same formulas at 50 digits, which sets the device tolerance; the matrices of every
category; the +I+G4 mixture of the recipe."""
import functools

import numpy as np

from phylo_amd import rates as R
from treegrad_cases import branch_matrices

# Measured by test_treegrad_rates_cpu.py::test_reference_against_mpmath (section 13's recipe: N = 5, S = 8, gaps, 20 trees, a
# GTR-like Q and JC69; the mixture p_inv = 0.1 + Gamma4(alpha = 0.5), so sites with f_0 = 0 are among them): the worst
# |reference - 50-digit value| over every entry of grad, curv, drate and dweight, in units of (scale + |value|) 2^-53.  The test
# asserts that it stays at or below E_REF_RATES.  Measured: grad 1.86, curv 7.54, drate 2.60, dweight 1.58.
E_REF_RATES = 7.6
TOL_RATES = 8 * E_REF_RATES * 2.0 ** -53      # device against reference: |difference| <= TOL_RATES (scale + |value|)

MIX_I_G4 = R.rate_model(0.5, 4, 0.1)


def category_matrices(Q, blen, rates):
    """expm(Q rate[c] blen) by scipy: [C] + blen.shape + [4][4] for rates [C]"""
    blen = np.asarray(blen, dtype=np.float64)
    return np.array([branch_matrices(Q, r * blen) for r in np.asarray(rates, dtype=np.float64).reshape(-1)])


def eigen_matrices(Q, t):
    """expm(Q t) for t [...] through Q's eigenvectors (a reversible Q has real ones): [...][4][4], good to 1e-12 or so -- for
    preconditions over many thousands of branches, not for comparisons"""
    lam, V = np.linalg.eig(Q)
    Vi = np.linalg.inv(V)
    t = np.asarray(t, dtype=np.float64)
    return np.real(np.einsum('ij,...j,jk->...ik', V, np.exp(t[..., None] * lam), Vi))


def plain_site_values(child, blen, Q, prior, leaves, rates, weights):
    """m [S] of one tree by ordinary matrix products (eigen_matrices, no fma chain): for preconditions"""
    N = leaves.shape[0]
    x = [np.broadcast_to(leaves[i], (len(rates),) + leaves[i].shape) for i in range(N)]
    M = eigen_matrices(Q, np.asarray(rates)[:, None, None] * blen)
    for i in range(N - 1):
        x.append(np.einsum('csk,ckj->csj', x[child[i, 0]], M[:, i, 0]) * np.einsum('csk,ckj->csj', x[child[i, 1]], M[:, i, 1]))
    return np.einsum('c,csj,j->s', np.asarray(weights), x[-1], prior)


@functools.lru_cache(maxsize=None)
def large_case(n=11):
    """N = 512 balanced, S = 65, simulated along the tree (trees_edges_cases.large_strided, three topologies in turn), under 16
    categories (+I+G15): (g, child, blen, Q, rates, weights).  32 MiB of node store per workgroup: 8 workgroups."""
    import trees_edges_cases as EC
    g, child, blen, Q = EC.large_strided(True, n)
    rates, weights = R.rate_model(0.5, 15, 0.1)
    return g, child, blen, Q, rates, weights


def simulate_rates(child, blen, Q, pi, S, rng, rates, weights):
    """an alignment [N][S][4] whose every site evolved down the tree at the rate of a category drawn by weight"""
    from treegrad_cases import simulate
    rates, weights = np.asarray(rates, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    cat = rng.choice(rates.size, size=S, p=weights / weights.sum())
    g = np.zeros((child.shape[0] + 1, S, 4))
    for c in range(rates.size):
        where = np.flatnonzero(cat == c)
        if where.size:
            g[:, where] = simulate(child, rates[c] * blen, Q, pi, where.size, rng)
    return g


def fit_case(N, S, n, seed, Q, pi, alpha=0.5, C=4):
    """an alignment simulated under Gamma-C(alpha) along a random tree (lengths + 0.05); that tree and n - 1 of its nearest-neighbour
    interchanges, every length off by a factor in [1/2, 2]: (g, child, blen)"""
    from test_gpu_treegrad import nni_neighbours
    from trees_cases import random_rows
    rng = np.random.default_rng(seed)
    c0, b0 = random_rows(N, rng, zeros=False)
    g = simulate_rates(c0, b0 + 0.05, Q, pi, S, rng, *R.rate_model(alpha, C))
    child = np.array(([c0] + nni_neighbours(c0))[:n])
    blen = (b0[None] + 0.05) * rng.uniform(0.5, 2.0, size=(child.shape[0], N - 1, 2))
    return g, child, blen
