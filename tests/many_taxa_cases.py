"""Inputs of the many-taxa tests (tests/test_gpu_grad_many_taxa.py, tests/test_many_taxa_cpu.py and the sharded worker
tests/_shard_grad_many_taxa_worker.py): coded synthetic alignments and models from seeded generators, so that every process of a
case -- the test, its worker ranks, the oracle -- builds the same arrays from (seed, N, S) alone."""
import numpy as np


def coded_alignment(seed, N, S):
    """[N, S, 4] leaves of codes A, C, G, T and gap (all ones), as tests/test_gpu_grad.py::_codes_genome draws them."""
    codes = np.random.default_rng(seed).integers(0, 5, size=(N, S))
    g = np.zeros((N, S, 4))
    for a in range(4):
        g[..., a] = (codes == a) | (codes == 4)
    return g


def random_model(seed, N, spread=0.3, lam=2.0):
    """(Q, pi[1, 4], lam_l, lam_r) as tests/test_gpu_grad.py::_model draws them."""
    rng = np.random.default_rng(seed)
    y = rng.normal(size=(4, 4)) * spread
    e = np.exp(y)
    np.fill_diagonal(e, 0.0)
    Q = e / e.sum(axis=1, keepdims=True)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    p = np.exp(rng.normal(size=4) * spread)
    pi = (p / p.sum())[None, :]
    return Q, pi, np.exp(rng.normal(size=N - 1) * spread + lam), np.exp(rng.normal(size=N - 1) * spread + lam)


def datadict(seed, N, S):
    """The reference's datadict ({'taxa', 'genome'}) of a coded alignment."""
    return {'taxa': ['S%d' % i for i in range(N)], 'genome': coded_alignment(seed, N, S)}
