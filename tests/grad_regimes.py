"""Model regimes for the whole reverse pass (TEST INFRASTRUCTURE ONLY): branch rates from 0.05 to 1e4 (branch lengths ~20 down to
~1e-4: the Frechet series at five to eight squarings, and at its shortest class), rates that differ by 1e4 between the sides and
between rank events, a skewed Q with a skewed stationary vector, generators that are not row-normalised, and the JC69 closed form.
tests/test_oracle_grad.py checks the gradient oracle against central differences on every regime (CPU); tests/test_gpu_grad.py runs
the device against the oracle on the same cases."""
import numpy as np

from oracle import cpu_ref as O


def _model(rng, N, spread=0.3, lam=2.0):
    """(the model of tests/test_gpu_grad.py::_model)"""
    y = rng.normal(size=(4, 4)) * spread
    e = np.exp(y)
    np.fill_diagonal(e, 0.0)
    Q = e / e.sum(axis=1, keepdims=True)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    p = np.exp(rng.normal(size=4) * spread)
    pi = (p / p.sum())[None, :]
    return Q, pi, np.exp(rng.normal(size=N - 1) * spread + lam), np.exp(rng.normal(size=N - 1) * spread + lam)


def _codes_genome(rng, N, S):
    codes = rng.integers(0, 5, size=(N, S))
    g = np.zeros((N, S, 4))
    for a in range(4):
        g[..., a] = (codes == a) | (codes == 4)
    return g


# name: (seed, N, S, K, generic leaves)
REGIMES = {
    'long_lam0.05': (301, 6, 40, 16, False),
    'long_lam0.3': (302, 7, 300, 48, False),               # two site tiles, ragged
    'unit_lam1': (303, 6, 40, 16, True),
    'short_lam500': (304, 8, 64, 24, False),
    'short_lam1e4': (305, 6, 40, 16, True),
    'mixed_left0.1_right1000': (306, 7, 65, 32, False),
    'mixed_alternating': (307, 8, 40, 16, False),
    'skewed_lam0.3': (308, 6, 40, 16, False),
    'skewed_lam7.4': (309, 7, 130, 24, True),
    'unnormalised_x30': (310, 6, 40, 16, False),
    'unnormalised_x1e-3': (311, 6, 64, 20, True),
    'jc69_lam0.05': (312, 6, 40, 16, False),
    'jc69_lam1e4': (313, 7, 65, 24, False),
}
SWITCH_REGIMES = ('long_lam0.05', 'skewed_lam0.3')          # also run with the host-built lists, eager nodes and the per-event chains


def regime(name):
    """-> dict(genome, Q, pi, ll, lr, K, seed, jc)."""
    seed, N, S, K, generic = REGIMES[name]
    rng = np.random.default_rng(seed)
    genome = rng.uniform(0.05, 1.0, size=(N, S, 4)) if generic else _codes_genome(rng, N, S)
    jc = name.startswith('jc69')
    kind, _, what = name.partition('_')
    if kind in ('long', 'unit', 'short'):
        Q, pi, ll, lr = _model(rng, N, spread=0.3, lam=np.log(float(what[3:])))
    elif name == 'mixed_left0.1_right1000':
        Q, pi, _, _ = _model(rng, N)
        ll, lr = np.full(N - 1, 0.1), np.full(N - 1, 1000.0)
    elif name == 'mixed_alternating':
        Q, pi, _, _ = _model(rng, N)
        ll = np.where(np.arange(N - 1) % 2 == 0, 0.1, 1000.0)
        lr = ll.copy()
    elif kind == 'skewed':
        Q, pi, ll, lr = _model(rng, N, spread=2.5, lam=np.log(float(what[3:])))
    elif kind == 'unnormalised':
        Q, pi, _, _ = _model(rng, N)
        Q = Q * float(what[1:])
        ll, lr = np.full(N - 1, 10.0), np.full(N - 1, 10.0)
    else:
        Q, pi = O.jc_Q(), np.full((1, 4), 0.25)
        ll, lr = np.full(N - 1, float(what[3:])), np.full(N - 1, float(what[3:]))
    return dict(genome=genome, Q=Q, pi=pi, ll=ll, lr=lr, K=K, seed=1000 + seed, jc=jc)
