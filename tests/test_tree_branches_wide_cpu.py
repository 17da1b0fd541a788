"""What tests/test_gpu_tree_branches_wide.py::test_wide_by_size stands on, without a GPU (tests/tree_branches_wide_cases.py):
the oracle's own sweep at the chosen shape and seed ends on enough clades and topologies that phylo_tree_branches takes 64-bit keys
by itself (a shape that falls short fails HERE instead of leaving the GPU test vacuous), and the array restatement of the branch
reference that the GPU test uses at that shape equals tests/tree_branches_ref.py bit for bit where that one is quick."""
import numpy as np
import pytest

import tree_branches_ref as BR
import tree_branches_wide_cases as WC
import tree_posterior_ref as REF
from oracle import c_oracle as CO
from oracle import cpu_ref as O
from phylo_amd import _ffi
from phylo_amd.datasets import load_dataset, synthetic_alignment

PI = np.full((1, 4), 0.25)


def oracle_sweep(g, K, seed):
    lam = np.full(g.shape[0] - 1, 10.0)
    return CO.sweep(g, O.jc_Q(), PI, lam, lam, K, seed, jc=True)


def test_the_shape_is_wide_by_itself():
    N, K, seed = WC.N, WC.K, WC.SEED
    out = oracle_sweep(WC.genome(), K, seed)
    assert not np.isfinite(out['log_weights']).any()        # no finite log-weight: every draw uniform, every u_k = 1
    clades = REF.particle_clades(N, K, out['merges'], out['ancestors'], seed, False)
    nc, nt = len({c for cl in clades for c in cl}), len({frozenset(cl) for cl in clades})
    assert (nc, nt) == WC.counts(N, K, out, seed)
    plan = _ffi.debug_tree_plan(N, K, n_clades=nc, n_topologies=nt)     # no switch
    print("N = %d K = %d seed %d: %d clades, %d topologies, cbits %d + tbits %d" % (N, K, seed, nc, nt, plan['cbits'], plan['tbits']))
    assert plan['wide'] and plan['cbits'] + plan['tbits'] > 32
    assert nt > 1 << 15 and nc > 1 << 14                    # topology rows set key bit cbits + 15 >= 32; clade rows use bit 14
    assert not _ffi.debug_tree_plan(N, K, n_clades=nc, n_topologies=1 << (32 - plan['cbits']))['wide']


@pytest.mark.parametrize("name,K,seed", [
    ('zeros', 32, 1),          # every u_k = 1
    ('ones', 256, 2),          # many topologies of one particle
    ('primates', 200, 3),      # one topology in the end: segments of 200 elements (more than three columns of 64)
    ('primates', 64, 4),       # segments of exactly 64
    ('primates', 65, 5),       # ... and 65
    ('zero-weight', 256, 1),   # clades held only by particles of weight 0
])
def test_the_array_reference_equals_tree_branches_ref(name, K, seed):
    g = {'zeros': lambda: np.zeros((8, 30, 4)), 'ones': lambda: np.ones((12, 50, 4)),
         'primates': lambda: load_dataset('primate_data_wang')['genome'],
         'zero-weight': lambda: synthetic_alignment(10, 150, seed=160)['genome']}[name]()
    N = g.shape[0]
    out = oracle_sweep(g, K, seed)
    summary, exp, _, u = BR.expected(out, N, K, seed)
    fsum, fexp = WC.fast_expected(out, N, K, seed)
    REF.assert_tables_equal(fsum, summary, name)
    BR.assert_branches_equal(fexp, exp, name)
    lens = sorted({len(m) for m in exp['clade_members']} | {len(m) for m in exp['topo_members']})
    print(name, K, "segment lengths", lens[:4], "...", lens[-1], "topologies", len(exp['topo_members']), "zero weights", u.count(0))
    if name == 'ones':
        assert len(exp['topo_members']) > 10 and 1 in lens
    if name == 'zero-weight':
        assert u.count(0) > 0 and (np.asarray(summary['clade_weight']) == 0).any()
    if name == 'primates':
        assert lens[-1] == K


def test_segment_sums_equal_canon_sum():
    rng = np.random.default_rng(7)
    lens = np.array([1, 2, 63, 64, 65, 127, 128, 129, 1000, 4097])
    starts = np.r_[0, np.cumsum(lens)[:-1]]
    x = rng.uniform(0.0, 1.0, lens.sum()) * 10.0 ** rng.integers(-8, 8, lens.sum())
    got = WC.segment_sums(x, starts, lens)
    want = np.array([BR.canon_sum(x[s:s + n]) for s, n in zip(starts, lens)])
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
