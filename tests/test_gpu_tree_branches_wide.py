"""The wide form of the branch pass (phylo_tree_branches with 64-bit (topology row, clade row) keys: pb_entry_keys<u64>, the 64-bit
rocPRIM sort, pb_seg_sums<PB_TOPOS, u64>, tperm in kA, two more buffers in the slab) on the device.

PHYLO_TREE_WIDE_KEYS=1 takes the wide form at any size and changes nothing else of the plan, so the
smallest cases of tests/test_gpu_tree_branches.py that stress the topology stage run it here: the forced-wide tables equal
tests/tree_branches_ref.py, the tables of a second context without the switch, and the contract's bounds, all bit for bit.
Every pass compared here is asked through phylo_debug_tree_branches_of which form it took: a switch that is not read fails the
test on that assertion.  The switch is read when a context is created, so it is set before the context is made.

One case is wide by size, with no switch (key bits above 31 are set only there): tests/test_tree_branches_wide_cpu.py pins, without
a GPU, that its shape needs more than 32 key bits under the oracle's own sweep."""
import time

import numpy as np
import pytest

import test_gpu_tree_branches as TB
import tree_branches_ref as BR
import tree_branches_wide_cases as WC
import tree_posterior_ref as REF
from phylo_amd import _ffi
from phylo_amd import treepost as TP
from phylo_amd.datasets import load_dataset, synthetic_alignment

pytestmark = pytest.mark.gpu
SWITCH = 'PHYLO_TREE_WIDE_KEYS'
SUMMARY = ('clade_bits', 'clade_weight', 'clade_group', 'topo_weight', 'topo_count', 'topo_rep', 'topo_group', 'particle_topo', 'u', 'U')


def tables(ctx, wide):
    """summary and branch tables of the context's last sweep; the pass must have taken the form claimed"""
    tab = TB.both(ctx)
    plan = ctx.debug_tree_branches()
    assert plan['wide'] is wide, "the branch pass took %r (PHYLO_TREE_WIDE_KEYS %s)" % (plan, "set" if wide else "unset")
    if not wide:
        assert plan['cbits'] + plan['tbits'] <= 32
    return tab


def same_tables(a, b, what):
    for key in SUMMARY:
        np.testing.assert_array_equal(np.asarray(a[key]), np.asarray(b[key]), err_msg="%s %s" % (what, key))
    for key in TB.STATS:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.shape == y.shape, (what, key)
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        np.testing.assert_array_equal(x, y, err_msg="%s %s" % (what, key))


def wide_vs_ref_and_narrow(monkeypatch, g, K, seed, flags=_ffi.FLAGS_DEFAULT, M=1, contract=True):
    """One sweep on a context made under the switch and one on a context made without it: the forced-wide tables against the
    reference (and the contract's bounds), the narrow tables against the forced-wide ones.  Returns the forced-wide group table."""
    N = g.shape[0]
    monkeypatch.setenv(SWITCH, '1')
    with TB.make_ctx(g, K) as ctx:
        out = ctx.sweep(seed, flags=flags, M=M)
        wide = tables(ctx, True)
    monkeypatch.delenv(SWITCH)
    with TB.make_ctx(g, K) as ctx:
        ctx.sweep(seed, flags=flags, M=M)
        narrow = tables(ctx, False)
    what = "forced wide K=%d seed=%d flags=%d" % (K, seed, flags)
    got = TP.group_table(wide, 0)
    summary, exp, trees, u = BR.expected(out, N, K, seed, twisted=bool(flags & _ffi.TWISTING))
    REF.assert_tables_equal(got, summary, what)
    BR.assert_branches_equal(got, exp, what)
    assert got['topo_clades'].shape == (len(got['topo_weight']), N - 2) and got['topo_stats'].shape[1:] == (2 * N - 2, 4)
    same_tables(narrow, wide, what + " against the narrow pass")
    if contract:
        TB.check_contract(got, exp, trees, u, N)
    return got


@pytest.mark.parametrize("K,seed", [(16, 0), (100, 3)])      # K not a multiple of 64
def test_forced_wide_primates(monkeypatch, K, seed):
    wide_vs_ref_and_narrow(monkeypatch, load_dataset('primate_data_wang')['genome'], K, seed)


def test_forced_wide_three_taxa_one_clade(monkeypatch):
    got = wide_vs_ref_and_narrow(monkeypatch, synthetic_alignment(3, 20, seed=3)['genome'], 96, 5)
    assert got['topo_clades'].shape[1] == 1 and got['topo_stats'].shape[1] == 4       # L = 1: one run per topology


def test_forced_wide_flat_weights_many_topologies(monkeypatch):
    got = wide_vs_ref_and_narrow(monkeypatch, np.ones((12, 50, 4)), 256, 2)
    assert len(got['topo_weight']) > 10 and (got['topo_count'] == 1).any()            # many topologies, segments of one particle


def test_forced_wide_a_clade_of_weight_zero(monkeypatch):
    got = wide_vs_ref_and_narrow(monkeypatch, synthetic_alignment(10, 150, seed=160)['genome'], 256, 1)
    zero = np.flatnonzero(got['clade_weight'] == 0)
    assert (got['u'] == 0).any() and zero.size > 0
    assert (got['clade_stats'][zero, :2] == 0.0).all() and (got['clade_stats'][zero, 2] > 0.0).all()


def test_forced_wide_all_bad_weights(monkeypatch):
    got = wide_vs_ref_and_narrow(monkeypatch, np.zeros((8, 30, 4)), 32, 1)
    assert (got['u'] == 1).all()


def test_forced_wide_two_bitset_words(monkeypatch):
    wide_vs_ref_and_narrow(monkeypatch, synthetic_alignment(70, 40, seed=70)['genome'], 64, 7)   # W = 2: cid and cpos do not depend on W


def test_forced_wide_twisted_proposal(monkeypatch):
    g = load_dataset('primate_data_wang')['genome']
    wide_vs_ref_and_narrow(monkeypatch, g, 32, 5, flags=_ffi.FLAGS_DEFAULT | _ffi.TWISTING, M=3)


def test_forced_wide_batched_groups_equal_single_sweeps(monkeypatch):
    g = load_dataset('primate_data_wang')['genome']
    seeds, Kg = [11, 22, 33, 44], 64
    G = len(seeds)
    monkeypatch.setenv(SWITCH, '1')
    with TB.make_ctx(g, G * Kg) as ctx:
        ctx.sweep_batch_async(seeds)
        wide = tables(ctx, True)
    monkeypatch.delenv(SWITCH)
    with TB.make_ctx(g, G * Kg) as ctx:
        ctx.sweep_batch_async(seeds)
        narrow = tables(ctx, False)
    assert wide['G'] == G and wide['leaf_stats'].shape == (G, g.shape[0], 4)
    same_tables(narrow, wide, "batch against the narrow pass")
    for gi, seed in enumerate(seeds):
        with TB.make_ctx(g, Kg) as single:
            out = single.sweep(seed)
            one = TP.group_table(tables(single, False), 0)
        grp = TP.group_table(wide, gi)
        REF.assert_tables_equal(grp, one, "group %d" % gi)
        BR.assert_branches_equal(grp, one, "group %d" % gi)
        summary, exp, _, _ = BR.expected(out, g.shape[0], Kg, seed)
        REF.assert_tables_equal(grp, summary, "group %d against the reference" % gi)
        BR.assert_branches_equal(grp, exp, "group %d against the reference" % gi)


@pytest.mark.parametrize("keep", [True, False])             # (without the kept graph the gather's two buffers lie beside wA / wB)
def test_forced_wide_sharded_ranks_return_the_unsharded_narrow_tables(monkeypatch, keep):
    g = load_dataset('primate_data_wang')['genome']
    K, seed = 64, 4
    with TB.make_ctx(g, K) as ctx:
        ctx.sweep(seed)
        one = tables(ctx, False)
    monkeypatch.setenv(SWITCH, '1')                         # run_world hands the environment on to the workers
    ranks = TB.run_world(2, K, 'primate_data_wang', seed, keep)
    assert len(ranks) == 2
    for r, t in enumerate(ranks):
        assert int(t['branch_plan'][0]) == 1, "rank %d took the narrow form: %r" % (r, t['branch_plan'])
        for key in ('clade_bits', 'clade_weight', 'topo_weight', 'particle_topo', 'u') + TB.STATS:
            a, b = t[key], one[key]
            if a.dtype == np.float64:
                a, b = a.view(np.uint64), b.view(np.uint64)
            np.testing.assert_array_equal(a, b, err_msg="rank %d %s" % (r, key))


def test_forced_wide_repeats_and_leaves_the_next_sweep_alone(monkeypatch):
    """tree_branches twice on one context: the same tables (the wide form sorts into kA and reads cpos again; the second pass finds
    both as the first left them).  Then the next sweep has the bits of a context that never ran the pass."""
    g = load_dataset('primate_data_wang')['genome']
    monkeypatch.setenv(SWITCH, '1')
    a, b = TB.make_ctx(g, 100), TB.make_ctx(g, 100)
    a.sweep(3)
    ta = a.tree_summary()
    first = a.tree_branches(ta)
    assert a.debug_tree_branches()['wide'] is True
    again = a.tree_branches(ta)
    assert a.debug_tree_branches()['wide'] is True
    for key in TB.STATS:
        x, y = first[key], again[key]
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        np.testing.assert_array_equal(x, y, err_msg=key)
    with pytest.raises(_ffi.PhyloError) as e:               # b has run no branch pass: there is no plan to report
        b.debug_tree_branches()
    assert e.value.code == -6
    b.sweep(3)
    ra, rb = a.sweep(2), b.sweep(2)
    for key in ('log_weights', 'log_likelihood', 'left_branches', 'right_branches'):
        assert np.array_equal(ra[key].view(np.uint64), rb[key].view(np.uint64)), key
    assert np.array_equal(ra['ancestors'], rb['ancestors']) and np.array_equal(ra['merges'], rb['merges']) and ra['logZ'] == rb['logZ']
    a.close()
    b.close()


def test_wide_by_size():
    """No switch: the shape of tests/tree_branches_wide_cases.py needs more than 32 key bits by itself, so topology rows from 2^15
    on set key bits above 31.  Every table is compared whole, topo_stats included: the array restatement of the reference
    (WC.fast_expected, held to tests/tree_branches_ref.py by tests/test_tree_branches_wide_cpu.py) takes seconds for all rows.
    Measured on an MI355X: 2.6 s for the test, of which 0.03 s are the context, the sweep, the two passes and their fetches (the
    branch pass: 1.24 ms on the device) and 2.5 s the reference on the host (7.4 s on a slower host without a GPU)."""
    N, K, seed = WC.N, WC.K, WC.SEED
    t0 = time.time()
    with TB.make_ctx(WC.genome(), K) as ctx:
        out = ctx.sweep(seed)
        tab = TB.both(ctx)
        plan = ctx.debug_tree_branches()
    t1 = time.time()
    assert plan['wide'] is True and plan['cbits'] + plan['tbits'] > 32
    got = TP.group_table(tab, 0)
    summary, exp = WC.fast_expected(out, N, K, seed)
    print("wide by size: context, sweep, summary, branch pass and fetches %.2f s (branch pass %.3f ms on the device), reference %.2f s, "
          "plan %r, %d clades, %d topologies" % (t1 - t0, tab['branches_ms'], time.time() - t1, plan, len(got['clade_weight']),
                                                len(got['topo_weight'])))
    nt = len(got['topo_weight'])
    assert nt > 1 << 15 and (got['topo_count'] > 1).any() and (got['u'] == 1).all()
    REF.assert_tables_equal(got, summary, "wide by size")
    BR.assert_branches_equal(got, exp, "wide by size")
