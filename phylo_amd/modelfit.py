"""The project's own parametrisation of the substitution model (phylo_amd.model: get_Q, the row-softmax of y_q off the diagonal;
get_stationary_probs, the softmax of y_station) as directions and chain rules for Context.trees_grad_model (DESIGN.md section
13c).  Pure NumPy, exact formulas of the softmax -- no differences.  No device code here."""
import numpy as np

from . import model

OFFDIAG = [(a, b) for a in range(4) for b in range(4) if a != b]      # the order of the twelve free entries of y_q


def q_directions(y_q):
    """The 12 directions dQ / d y_q[a][b], a != b, in OFFDIAG's order: [12][4][4].  Row a of get_Q is the softmax q of y_q[a] over
    its off-diagonal entries, so d q[a][c] / d y_q[a][b] = q[a][c] ((b == c) - q[a][b]) for c != a, every other row is 0, and the
    diagonal entry follows as minus the sum of its row."""
    Q = model.get_Q(y_q)
    out = np.zeros((len(OFFDIAG), 4, 4))
    for p, (a, b) in enumerate(OFFDIAG):
        for c in range(4):
            if c != a:
                out[p, a, c] = Q[a, c] * ((1.0 if c == b else 0.0) - Q[a, b])
        out[p, a, a] = -sum(out[p, a, c] for c in range(4) if c != a)
    return out


def pack_q(y_q):
    """the twelve free coordinates of y_q in OFFDIAG's order"""
    y_q = np.asarray(y_q, dtype=np.float64)
    return np.array([y_q[a, b] for a, b in OFFDIAG])


def unpack_q(v):
    """y_q [4][4] with a zero diagonal from its twelve free coordinates"""
    y = np.zeros((4, 4))
    for p, (a, b) in enumerate(OFFDIAG):
        y[a, b] = v[p]
    return y


def chain_prior(dprior, y_station):
    """d loglik / d y_station [..., 4] from dprior [..., 4] = d loglik / d prior at prior = softmax(y_station):
    d pi[j] / d y[k] = pi[j] ((j == k) - pi[k]), so the result is pi[k] (dprior[k] - sum_j pi[j] dprior[j])."""
    pi = model.get_stationary_probs(y_station).reshape(4)
    dprior = np.asarray(dprior, dtype=np.float64)
    return pi * (dprior - (dprior * pi).sum(axis=-1, keepdims=True))
