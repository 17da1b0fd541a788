"""The tree posterior summary on the device (phylo_tree_summary) against tests/tree_posterior_ref.py, which rebuilds every
particle's clades from the fetched merges and ancestors: bitsets, u64 weights, counts, representatives and per-particle
topologies equal exactly, for every sweep form, batched groups, 1 / 2 / 3 ranks, and through VCSMC and runner.py."""
import glob
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import tree_posterior_ref as REF
from phylo_amd import _ffi, model
from phylo_amd import treepost as TP
from phylo_amd.datasets import load_dataset, synthetic_alignment
from phylo_amd.vcsmc import VCSMC, default_args

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PI = np.full((1, 4), 0.25)


def make_ctx(g, K, jc=True):
    N, S, _ = g.shape
    ctx = _ffi.Context(K, N, S)
    ctx.set_leaves(g)
    Q = model.jc_Q() if jc else model.get_Q(model.init_y_q())
    lam = np.full(N - 1, 10.0)
    ctx.set_model(Q, PI, lam, lam, jc69_closed_form=jc)
    return ctx


def expected(out, N, K, seed, twisted=False):
    clades = REF.particle_clades(N, K, out['merges'], out['ancestors'], seed, twisted)
    return REF.summarise(N, clades, REF.int_weights(out['log_weights'][N - 2])), clades


def check_invariants(t, N, K):
    U = int(t['U'])
    assert sum(int(c) for c in t['clade_weight']) == (N - 2) * U
    assert sum(int(x) for x in t['topo_weight']) == U
    assert int(np.sum(t['topo_count'])) == K
    assert sum(int(x) for x in t['u']) == U


def summary_vs_ref(g, K, seed, jc=True, flags=_ffi.FLAGS_DEFAULT, M=1):
    N = g.shape[0]
    ctx = make_ctx(g, K, jc)
    out = ctx.sweep(seed, flags=flags, M=M)
    tab = ctx.tree_summary()
    ctx.close()
    got = TP.group_table(tab, 0)
    exp, _ = expected(out, N, K, seed, twisted=bool(flags & _ffi.TWISTING))
    REF.assert_tables_equal(got, exp, "K=%d seed=%d flags=%d" % (K, seed, flags))
    check_invariants(got, N, K)
    assert tab['G'] == 1 and tab['W'] == (N + 63) // 64
    return got


@pytest.mark.parametrize("dataset,K,seeds,jc", [
    ('primate_data_wang', 16, (0,), True),          # primates_small JC69
    ('primate_data', 2048, (0, 1, 2, 3), False),    # primate.p GTR
    ('hohna_data_1', 4096, (0,), True),             # DS1
])
def test_summary_equals_reference(dataset, K, seeds, jc):
    g = load_dataset(dataset)['genome']
    for seed in seeds:
        summary_vs_ref(g, K, seed, jc=jc)


@pytest.mark.parametrize("N,K", [(70, 64), (130, 16)])     # W = 2 (a word boundary), W = 3
def test_summary_multiword_bitsets(N, K):
    g = synthetic_alignment(N, 40, seed=N)['genome']
    got = summary_vs_ref(g, K, 7)
    assert got['clade_bits'].shape[1] == (N + 63) // 64
    assert (got['clade_bits'][:, -1] != 0).any()           # taxa past the first word(s) are there


def test_summary_flat_workload_many_survivors():
    g = np.ones((12, 50, 4))                               # all-gap rows: every weight equal, many particles survive
    got = summary_vs_ref(g, 256, 2)
    assert len(got['topo_weight']) > 10


def test_summary_all_bad_final_row():
    g = np.zeros((8, 30, 4))                               # no finite log-weight anywhere: every u_k = 1
    got = summary_vs_ref(g, 32, 1)
    assert (got['u'] == 1).all() and got['U'] == 32


@pytest.mark.parametrize("M", [1, 3])
def test_summary_twisted_proposal(M):
    g = load_dataset('primate_data_wang')['genome']
    summary_vs_ref(g, 32, 5, flags=_ffi.FLAGS_DEFAULT | _ffi.TWISTING, M=M)


def test_batched_groups_equal_single_sweeps():
    g = load_dataset('primate_data_wang')['genome']
    G, Kg = 4, 64
    seeds = [11, 22, 33, 44]
    ctx = make_ctx(g, G * Kg)
    ctx.sweep_batch_async(seeds)
    tab = ctx.tree_summary()
    ctx.close()
    assert tab['G'] == G
    for gi, seed in enumerate(seeds):
        single = make_ctx(g, Kg)
        single.sweep(seed)
        one = TP.group_table(single.tree_summary(), 0)
        single.close()
        REF.assert_tables_equal(TP.group_table(tab, gi), one, "group %d" % gi)


def test_one_launch_and_eager_nodes_give_the_default_table():
    g = load_dataset('primate_data_wang')['genome']
    tabs = []
    for flags in (_ffi.FLAGS_DEFAULT, _ffi.FLAGS_DEFAULT | _ffi.ONE_LAUNCH, _ffi.FLAGS_DEFAULT | _ffi.EAGER_NODES):
        ctx = make_ctx(g, 128)
        ctx.sweep(9, flags=flags)
        tabs.append(TP.group_table(ctx.tree_summary(), 0))
        ctx.close()
    for t in tabs[1:]:
        REF.assert_tables_equal(t, tabs[0])


def test_summary_leaves_the_next_sweep_alone():
    g = load_dataset('primate_data_wang')['genome']
    a, b = make_ctx(g, 64), make_ctx(g, 64)
    a.sweep(1)
    a.tree_summary()
    ra = a.sweep(2)
    b.sweep(1)
    rb = b.sweep(2)
    for key in ('log_weights', 'log_likelihood', 'left_branches'):
        assert np.array_equal(ra[key].view(np.uint64), rb[key].view(np.uint64)), key
    assert np.array_equal(ra['ancestors'], rb['ancestors']) and ra['logZ'] == rb['logZ']
    a.close()
    b.close()


def test_summary_needs_a_sweep():
    g = load_dataset('primate_data_wang')['genome']
    ctx = make_ctx(g, 16)
    with pytest.raises(_ffi.PhyloError) as e:
        ctx.tree_summary()
    assert e.value.code == -6
    ctx.close()


def test_vcsmc_tree_posterior_newick_and_consensus():
    d = load_dataset('primate_data_wang')
    v = VCSMC(d, K=256, args=default_args(jcmodel=True, seed=3))
    v.sample_phylogenies()
    post = v.tree_posterior()
    N = v.N
    _, clades = expected({'merges': v.merges, 'ancestors': v.ancestors, 'log_weights': v.log_weights}, N, v.K, v._last_seed)
    for t in post.topologies:
        want = {frozenset(i for i in range(N) if c >> i & 1) for c in clades[t['representative']]}
        assert TP.newick_clades(t['newick'], v.taxa) == want
    assert abs(sum(t['probability'] for t in post.topologies) - 1.0) < 1e-12
    assert post.map is post.topologies[0]
    assert TP.newick_clades(post.consensus, v.taxa) == {m for m, s in post.clade_sets if s > 0.5}
    assert post.credible_set(1.0) == post.topologies[:len(post.credible_set(1.0))]
    v.close()


def run_world(world, K, dataset, seed):
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, PHYLO_RDZV_DIR=tmp, MASTER_PORT=str(29300 + os.getpid() % 600 + world), PHYLO_COMM='hostshm')
        procs = []
        for r in range(world):
            out = os.path.join(tmp, "r%d.npz" % r)
            procs.append((out, subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_tree_summary_worker.py"), str(r),
                                                 str(world), str(K), dataset, str(seed), out],
                                                env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        outs = []
        for out, p in procs:
            try:
                log, _ = p.communicate(timeout=240)
            except subprocess.TimeoutExpired:
                for _, q in procs:
                    q.kill()
                raise
            assert p.returncode == 0, log.decode()[-2000:]
            outs.append(dict(np.load(out)))
        return outs


@pytest.mark.parametrize("world,K", [(2, 64), (3, 96)])
def test_sharded_ranks_return_the_unsharded_table(world, K):
    g = load_dataset('primate_data_wang')['genome']
    ctx = make_ctx(g, K)
    ctx.sweep(4)
    one = ctx.tree_summary()
    ctx.close()
    for t in run_world(world, K, 'primate_data_wang', 4):
        for key in ('clade_bits', 'clade_weight', 'clade_group', 'topo_weight', 'topo_count', 'topo_rep', 'topo_group',
                    'particle_topo', 'u', 'U'):
            np.testing.assert_array_equal(t[key], one[key], err_msg=key)


def test_runner_tree_summary_writes_the_files():
    argv = ['--dataset', 'primate_data_wang', '--n_particles', '16', '--num_epoch', '2', '--jcmodel', 'true', '--seed', '2']
    keys = []
    for extra in (['--tree_summary', 'true'], []):
        with tempfile.TemporaryDirectory() as tmp:
            p = subprocess.run([sys.executable, os.path.join(ROOT, 'runner.py')] + argv + extra, cwd=tmp,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
            assert p.returncode == 0, p.stdout.decode()[-2000:]
            (res,) = glob.glob(os.path.join(tmp, 'results', '*', '*', '*', '*', 'results.p'))
            d = os.path.dirname(res)
            with open(res, 'rb') as f:
                keys.append(sorted(pickle.load(f)))
            files = os.path.exists(os.path.join(d, 'tree_posterior.json')), os.path.exists(os.path.join(d, 'consensus.tre'))
            if extra:
                assert files == (True, True)
                taxa = load_dataset('primate_data_wang')['taxa']
                with open(os.path.join(d, 'consensus.tre')) as f:
                    TP.newick_clades(f.read().strip(), taxa)          # parses
            else:
                assert files == (False, False)
    assert keys[0] == keys[1]
