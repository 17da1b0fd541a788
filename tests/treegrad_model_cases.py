"""Shared inputs of the model-gradient tests: the simulated 8-taxon case of the model fit, the functions
that drive phylo_amd.treeopt.optimize_model from the NumPy restatements, and the figures the CPU test measured on them."""
import functools

import numpy as np

import treegrad_model_ref as MR
import treegrad_ref as TR
from phylo_amd import model
from treegrad_cases import branch_matrices, simulate
from trees_cases import random_rows

# Measured by test_treegrad_model_cpu.py::test_optimize_model_against_lbfgsb on fit_case() under the textbook convention: scipy's
# L-BFGS-B on the joint function (model coordinates and the lengths of the fit_on tree) from two starts agrees with itself to
# 4.7e-16 relative in the objective.  That is below the rounding of a sum over 600 sites, about 2^-46 of its size (what
# treeopt.NOISE takes for it, and the bound section 13's optimiser test holds both agreements to): FIT_MARGIN is 2^-46.
FIT_MARGIN = 2.0 ** -46
# The objective optimize_model reaches on fit_case() under the project's OWN convention with fit=('q', 'pi'), converged (16 rounds),
# from the starting model below, driven by the restatements (asserted within FIT_MARGIN by
# test_treegrad_model_cpu.py::test_optimize_model_under_the_projects_convention; the device test compares its own fit
# with this number and needs no host fit).  It lies 1159 above the objective of the model the data were simulated under:
# there the site factors of an asymmetric Q do not sum to one over the columns and the objective has no interior maximum (the
# fit ends at pi = (0, 1, 0, 0) and a Q whose rows hold one entry each).  DESIGN.md section 13c says what that means.
FIT_OBJECTIVE_HOST = -3183.415096704375


def nni_neighbours(child):
    """the trees one nearest-neighbour interchange away from child (those whose rows stay children-first)"""
    R = child.shape[0]
    N = R + 1
    parent = {int(child[p, sd]): (p, sd) for p in range(R) for sd in range(2)}
    out = []
    for i in range(R - 1):
        p, sd = parent[N + i]
        s = child[p, 1 - sd]
        if s < N + i:
            for k in range(2):
                c = child.copy()
                c[i, k], c[p, 1 - sd] = s, child[i, k]
                out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def fit_case():
    """8 taxa, 600 sites simulated along a random tree under a known row-softmax Q and pi; that tree and four of its NNI
    neighbours, every length off by a factor in [1/2, 2].  Returns a dict (treat it as read-only)."""
    N, S = 8, 600
    rng = np.random.default_rng(2024)
    y_q = rng.normal(scale=0.7, size=(4, 4))
    np.fill_diagonal(y_q, 0.0)
    y_station = rng.normal(scale=0.4, size=4)
    Q, pi = model.get_Q(y_q), model.get_stationary_probs(y_station).reshape(4)
    c0, b0 = random_rows(N, rng, zeros=False)
    b0 = b0 + 0.05
    g = simulate(c0, b0, Q, pi, S, rng)
    child = np.array([c0] + nni_neighbours(c0)[:4])
    assert child.shape[0] == 5
    blen = b0[None] * rng.uniform(0.5, 2.0, size=(5, N - 1, 2))
    return {'N': N, 'S': S, 'g': g, 'child': child, 'blen': blen, 'true_blen': b0, 'y_q': y_q, 'y_station': y_station, 'Q': Q, 'pi': pi,
            'y_q0': model.init_y_q(), 'y_station0': np.full(4, 0.25)}      # the values a VCSMC starts from


def host_fns(child, g, textbook=False):
    """grad_fn and grad_model_fn of optimize_model from the restatements (scipy's expm for the branch matrices).  textbook: the
    same restatements under the TEXTBOOK pruning convention, a message M . x_child: that is the project's x_child . M with every
    matrix transposed, i.e. with the generator Q^T (expm(Q^T t) = expm(Q t)^T, L(A^T, E^T) = L(A, E)^T, M^T Q^T = (M Q)^T).  Its
    site factors are probabilities for every Q with zero row sums, which is what get_Q makes."""
    def grad_fn(b, Q, pi):
        Qe = Q.T if textbook else Q
        ll, grad, curv, _ = TR.trees_grad(child, branch_matrices(Qe, b), Qe, pi, g)
        return ll, grad, curv

    def grad_model_fn(idx, b, Q, pi, dirs):
        Qe, de = (Q.T, np.ascontiguousarray(np.swapaxes(dirs, 1, 2))) if textbook else (Q, dirs)
        ll, dth, dpr, _, _ = MR.trees_grad_model(child[idx], branch_matrices(Qe, b), MR.direction_matrices(Qe, de, b), pi, g)
        return ll, dth, dpr

    return grad_fn, grad_model_fn
