"""Shapes of tests/test_gpu_book_widths.py: the bookkeeping at a wave per particle (pk_rank_book_packed<64>), which every sweep of
more than 32 taxa takes unless the combined launch (pk_rank_book_mat: one sweep alone, up to 64 taxa) is chosen, against the C
oracle.  Inputs are those of tests/many_taxa_cases.py: coded_alignment(1000 + N, N, S), random_model(2000 + N, N).
tests/test_book_widths_cpu.py pins the plan facts each case stands on.

  key-loop          257 taxa: the first five rank events have 65 .. 64 Philox key blocks (n = 257 .. 253 root slots), more than the
                    63 lanes a wave has to spare beside its resampling counter: the strided key loop runs there, the single
                    evaluation from the sixth rank event on
  key-loop-batched  the same with two groups of 4: the group's base and its cdf segment at 64 lanes
  n65               the first N beyond the combined launch's limit
  n33-batched       the first N at 64 lanes, as a batch: the bookkeeping kernel runs, not the combined one
"""
import functools

import many_taxa_cases as MC
from oracle import c_oracle as CO

S = 8
CASES = {
    "key-loop":         dict(N=257, G=1, Kg=8, seeds=(5,)),
    "key-loop-batched": dict(N=257, G=2, Kg=4, seeds=(5, 15)),
    "n65":              dict(N=65, G=1, Kg=16, seeds=(5,)),
    "n33-batched":      dict(N=33, G=2, Kg=8, seeds=(5, 15)),
}
NAMES = list(CASES)

# two ranks on one GPU (tests/_shard_worker.py: GTR-init model, rates 10): DS3, 36 taxa -- owner-held tables at 64 lanes
SHARDED = dict(dataset="hohna_data_3", N=36, S=1812, world=2, K=16, seed=4)
# the twisted proposal's search (pk_twist_adopt_draws): one round of 64 probes
TWISTED = dict(N=5, K=64, S=64, M=1, seed=5)


@functools.lru_cache(maxsize=None)
def model(N, S=S):
    """(genome, Q, pi, lam_l, lam_r) of N taxa"""
    return (MC.coded_alignment(1000 + N, N, S),) + MC.random_model(2000 + N, N)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's sweep of every group of the case (computed once per process; do not modify)"""
    c = CASES[name]
    g, Q, pi, lam_l, lam_r = model(c["N"])
    return [CO.sweep(g, Q, pi, lam_l, lam_r, c["Kg"], seed) for seed in c["seeds"]]
