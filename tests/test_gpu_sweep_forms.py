"""What ties the plan of the forward sweep (phylo_sweep_plan.h, pinned without a GPU by test_sweepplan_cpu.py) to the driver that
issues it: at the smallest shape at which each form is selected, stats['n_launches'] equals the count recorded from the driver
as it was before there was a plan (HISTORY.md, "Forward sweep: one plan, named stages"), and log Z-hat is bit-equal between the
forms of the plain proposal at one shape and seed.  Each form's own parity with the oracle is asserted elsewhere
(test_gpu_parity.py, test_gpu_merge_record.py, test_gpu_fullsize.py)."""
import numpy as np
import pytest

from phylo_amd import _ffi
from phylo_amd.datasets import synthetic_alignment

pytestmark = pytest.mark.gpu

DEFAULT = _ffi.FLAGS_DEFAULT
SEED = 11

# (N, K, S) -> {form: n_launches}.  R = N - 1 rank events; a begin of one launch; the last scan also sums the log-normalisers.
LAUNCHES = {
    # bookkeeping (+ the adopted nodes in the same launch when lazy), merge, scan: 1 + 3 R
    (5, 64, 64): {"default": 13, "eager": 13, "graph": 13, "timed": 13},
    (17, 64, 64): {"default": 49, "eager": 49, "graph": 49},             # 32 lanes per particle
    (33, 16, 64): {"default": 97, "eager": 97, "graph": 97},             # 64 lanes per particle
    # beyond 64 taxa: one-wave bookkeeping and the adopted nodes in a launch of their own for r > 0: 1 + 3 + 4 (R - 1)
    (65, 16, 64): {"default": 256, "eager": 193, "graph": 256},
    # three site tiles: the tile epilogue behind every merge, no combined launch: 1 + 4 + 5 (R - 1); eager 1 + 4 R
    (5, 16, 4160): {"default": 20, "eager": 17},
}
TWISTED_LAUNCHES = 25                 # (5, 64, 64), M = 1, coded leaves: adopt + draws, two potentials, choose, merge, scan: 1 + 6 R
BATCHED_LAUNCHES = 16                 # (5, 64, 64), G = 2: the adopted nodes in a launch of their own for r > 0: 1 + 3 + 4 (R - 1)
FLAGS = {"default": DEFAULT, "eager": DEFAULT | _ffi.EAGER_NODES, "graph": DEFAULT | _ffi.KEEP_GRAPH, "timed": DEFAULT | _ffi.TIME_KERNELS}


def make_ctx(N, K, S):
    g = synthetic_alignment(N, S, seed=N + S)['genome']
    Q = np.array([[-1.0, 0.3, 0.5, 0.2], [0.3, -1.1, 0.2, 0.6], [0.5, 0.2, -1.0, 0.3], [0.2, 0.6, 0.3, -1.1]])
    ctx = _ffi.Context(K, N, S)
    ctx.set_leaves(g)
    ctx.set_model(Q, np.array([[0.1, 0.2, 0.3, 0.4]]), np.linspace(8.0, 12.0, N - 1), np.linspace(11.0, 9.0, N - 1))
    return ctx


@pytest.mark.parametrize("N,K,S", sorted(LAUNCHES))
def test_plain_forms_launch_counts_and_equal_bits(N, K, S):
    with make_ctx(N, K, S) as ctx:
        logz = {}
        for form, want in LAUNCHES[(N, K, S)].items():
            out = ctx.sweep(SEED, FLAGS[form])
            print("N=%d K=%d S=%d %s: n_launches %d logZ %r" % (N, K, S, form, out['stats']['n_launches'], out['logZ']))
            assert out['stats']['n_launches'] == want, form
            logz[form] = np.float64(out['logZ']).view(np.uint64)
        assert np.isfinite(out['logZ']) and len(set(logz.values())) == 1, logz


def test_twisted_launch_count():
    with make_ctx(5, 64, 64) as ctx:
        out = ctx.sweep(SEED, DEFAULT | _ffi.TWISTING, M=1)
        print("twisted: n_launches %d logZ %r" % (out['stats']['n_launches'], out['logZ']))
        assert out['stats']['n_launches'] == TWISTED_LAUNCHES and np.isfinite(out['logZ'])


def test_batched_launch_count_and_bits_of_each_sweep_alone():
    """G = 2 sweeps of 32 particles in one set of launches: each equals, bit for bit, the sweep of 32 particles with its seed"""
    with make_ctx(5, 64, 64) as ctx:
        ctx.sweep_batch_async([SEED, SEED + 1])
        logz = ctx.sweep_fetch_logz(2)
        n = ctx.sweep_fetch(arrays=False)['stats']['n_launches']
    print("batched: n_launches %d logZ %r" % (n, logz))
    assert n == BATCHED_LAUNCHES
    with make_ctx(5, 32, 64) as ctx:
        for g in range(2):
            assert np.float64(ctx.sweep(SEED + g)['logZ']).view(np.uint64) == logz[g].view(np.uint64)
