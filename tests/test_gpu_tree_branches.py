"""Branch lengths of the tree posterior on the device (phylo_tree_branches) against tests/tree_branches_ref.py, which rebuilds
every particle's tree and its branch lengths from the FETCHED merges, ancestors and left / right branches and restates the
canonical segment sum in NumPy: every table equal bit for bit, for every sweep form, batched groups and 1 / 2 / 3 ranks; the sums
within their derived bound of the exact sums; the state rules; VCSMC.tree_posterior(branch_lengths=True) and runner.py.

Every test here needs phylo_tree_branches: on a tree without it, Context.tree_branches raises AttributeError."""
import glob
import os
import pickle
import subprocess
import sys
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import tree_branches_ref as BR
import tree_posterior_ref as REF
from phylo_amd import _ffi, model
from phylo_amd import treepost as TP
from phylo_amd.datasets import load_dataset, synthetic_alignment
from phylo_amd.vcsmc import VCSMC, default_args

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PI = np.full((1, 4), 0.25)
STATS = ('clade_stats', 'leaf_stats', 'topo_stats', 'topo_clades')
EPS = 2.0 ** -53


def make_ctx(g, K, jc=True):
    N, S, _ = g.shape
    ctx = _ffi.Context(K, N, S)
    ctx.set_leaves(g)
    Q = model.jc_Q() if jc else model.get_Q(model.init_y_q())
    lam = np.full(N - 1, 10.0)
    ctx.set_model(Q, PI, lam, lam, jc69_closed_form=jc)
    return ctx


def both(ctx):
    tab = ctx.tree_summary()
    tab.update(ctx.tree_branches(tab))
    return tab


def check_contract(got, exp, trees, u, N):
    """Item 3: each S1, S2 within (ceil(n / 64) + 8) 2^-53 (relative) of the exact sum -- all terms are non-negative, a column is a
    recursive sum of ceil(n / 64) terms, the tree adds 6 levels, the products 2 roundings -- and min <= S1 / C <= max where C > 0.
    The mean is a rounded quotient of a rounded sum, so that comparison allows the sum's bound plus the division's rounding
    (a segment of one element has S1 / C = fl(fl(u b) / u), which need not be b itself).
    Then item 4's total: all clade and leaf S1 together are sum of u_k (tree length of k) within those bounds summed."""
    K = len(trees)
    slack = Fraction(0)

    def one(row, ks, key, weight):
        us, bs = [u[k] for k in ks], [trees[k][key][1] for k in ks]
        e1, e2 = BR.exact_sums(us, bs)
        rel = BR.bound(len(ks))
        assert abs(Fraction(float(row[0])) - e1) <= Fraction(rel) * e1, (key, len(ks), float(row[0]), float(e1))
        assert abs(Fraction(float(row[1])) - e2) <= Fraction(rel) * e2, (key, len(ks), float(row[1]), float(e2))
        assert row[2] == min(bs) and row[3] == max(bs)
        if weight > 0:
            assert weight == sum(us)
            mean = float(row[0]) / float(weight)
            assert row[2] * (1 - rel - EPS) <= mean <= row[3] * (1 + rel + EPS), (key, mean, row[2], row[3])
        return Fraction(rel) * e1

    for j, c in enumerate(exp['clade_keys']):
        slack += one(got['clade_stats'][j], exp['clade_members'][j], c, int(got['clade_weight'][j]))
    for i in range(N):
        slack += one(got['leaf_stats'][i], list(range(K)), 1 << i, int(got['U']))
    for t, ks in enumerate(exp['topo_members']):
        keys = [1 << i for i in range(N)] + [exp['clade_keys'][j] for j in got['topo_clades'][t]]
        for q, c in enumerate(keys):
            one(got['topo_stats'][t, q], ks, c, int(got['topo_weight'][t]))
    # item 4, second half: all the clade and leaf sums together are the weighted total tree length
    exact = sum(int(u[k]) * sum(Fraction(b) for _, b in trees[k].values()) for k in range(K))
    got_total = sum(Fraction(float(x)) for x in got['clade_stats'][:, 0]) + sum(Fraction(float(x)) for x in got['leaf_stats'][:, 0])
    assert abs(got_total - exact) <= slack, (float(got_total), float(exact), float(slack))


def branches_vs_ref(g, K, seed, jc=True, flags=_ffi.FLAGS_DEFAULT, M=1, contract=True):
    N = g.shape[0]
    ctx = make_ctx(g, K, jc)
    out = ctx.sweep(seed, flags=flags, M=M)
    tab = both(ctx)
    ctx.close()
    got = TP.group_table(tab, 0)
    summary, exp, trees, u = BR.expected(out, N, K, seed, twisted=bool(flags & _ffi.TWISTING))
    what = "K=%d seed=%d flags=%d" % (K, seed, flags)
    REF.assert_tables_equal(got, summary, what)
    BR.assert_branches_equal(got, exp, what)
    assert got['topo_clades'].shape == (len(got['topo_weight']), N - 2) and got['topo_stats'].shape[1:] == (2 * N - 2, 4)
    if contract:
        check_contract(got, exp, trees, u, N)
    return got, exp


@pytest.mark.parametrize("dataset,K,seeds,jc", [
    ('primate_data_wang', 16, (0,), True),          # primates_small JC69
    ('primate_data_wang', 100, (3,), True),         # K not a multiple of 64
    ('primate_data', 2048, (0, 1), False),          # primate.p GTR
    ('hohna_data_1', 4096, (0,), True),             # DS1
])
def test_branches_equal_reference(dataset, K, seeds, jc):
    g = load_dataset(dataset)['genome']
    for seed in seeds:
        branches_vs_ref(g, K, seed, jc=jc, contract=K <= 2048)


def test_a_clade_of_weight_zero_has_sums_but_no_mean():
    # 10 taxa, 150 random sites: most integer weights are 0 and the survivors still differ, so some clades are held only by
    # particles of weight 0 (an alignment such as primate.p ends on one topology: every clade there has weight U)
    g = synthetic_alignment(10, 150, seed=160)['genome']
    got, _ = branches_vs_ref(g, 256, 1)
    zero = np.flatnonzero(got['clade_weight'] == 0)
    assert (got['u'] == 0).any() and zero.size > 0
    assert (got['clade_stats'][zero, :2] == 0.0).all() and (got['clade_stats'][zero, 2] > 0.0).all()
    post = TP.TreePosterior(['t%d' % i for i in range(g.shape[0])], got)
    assert post.clade_branches[int(zero[0])]['mean'] is None and post.clade_branches[0]['mean'] is not None
    assert 'nan' not in (post.consensus_bl + post.map_newick).lower()


def test_three_taxa_one_clade():
    got, _ = branches_vs_ref(synthetic_alignment(3, 20, seed=3)['genome'], 96, 5)
    assert got['topo_clades'].shape[1] == 1 and got['topo_stats'].shape[1] == 4


@pytest.mark.parametrize("N,K", [(70, 64), (130, 16)])     # W = 2 (a word boundary), W = 3
def test_branches_multiword_bitsets(N, K):
    branches_vs_ref(synthetic_alignment(N, 40, seed=N)['genome'], K, 7)


def test_flat_and_all_bad_weights():
    got, _ = branches_vs_ref(np.ones((12, 50, 4)), 256, 2)           # every weight equal, many topologies
    assert len(got['topo_weight']) > 10
    got, _ = branches_vs_ref(np.zeros((8, 30, 4)), 32, 1)            # no finite log-weight: every u_k = 1
    assert (got['u'] == 1).all()


def test_a_segment_longer_than_64_columns_of_64():
    g = load_dataset('primate_data_wang')['genome']
    got, exp = branches_vs_ref(g, 8192, 6)                 # every leaf segment: 8192 elements = 128 per column
    assert got['leaf_stats'].shape == (g.shape[0], 4) and len(exp['topo_members']) == len(got['topo_weight'])


@pytest.mark.parametrize("M", [1, 3])
def test_branches_twisted_proposal(M):
    g = load_dataset('primate_data_wang')['genome']
    branches_vs_ref(g, 32, 5, flags=_ffi.FLAGS_DEFAULT | _ffi.TWISTING, M=M)


def test_one_launch_and_eager_nodes_give_the_default_tables():
    g = load_dataset('primate_data_wang')['genome']
    tabs = []
    for flags in (_ffi.FLAGS_DEFAULT, _ffi.FLAGS_DEFAULT | _ffi.ONE_LAUNCH, _ffi.FLAGS_DEFAULT | _ffi.EAGER_NODES):
        got, _ = branches_vs_ref(g, 128, 9, flags=flags, contract=False)
        tabs.append(got)
    for t in tabs[1:]:
        BR.assert_branches_equal(t, tabs[0])


def batch_vs_singles(g, seeds, Kg, jc=True):
    G = len(seeds)
    ctx = make_ctx(g, G * Kg, jc)
    ctx.sweep_batch_async(seeds)
    tab = both(ctx)
    ctx.close()
    assert tab['G'] == G and tab['leaf_stats'].shape == (G, g.shape[0], 4)
    for gi, seed in enumerate(seeds):
        single = make_ctx(g, Kg, jc)
        single.sweep(seed)
        one = TP.group_table(both(single), 0)
        single.close()
        grp = TP.group_table(tab, gi)
        REF.assert_tables_equal(grp, one, "group %d" % gi)
        BR.assert_branches_equal(grp, one, "group %d" % gi)


def test_batched_groups_equal_single_sweeps():
    batch_vs_singles(load_dataset('primate_data_wang')['genome'], [11, 22, 33, 44], 64)


def test_batched_primate_20_groups_of_2048():
    batch_vs_singles(load_dataset('primate_data')['genome'], [1 + 10 * i for i in range(20)], 2048, jc=False)


def test_state_rules_and_nothing_else_moves():
    g = load_dataset('primate_data_wang')['genome']
    a, b = make_ctx(g, 64), make_ctx(g, 64)
    for ctx in (a, b):
        with pytest.raises(_ffi.PhyloError) as e:           # no sweep, no summary
            ctx.tree_branches({'clade_weight': [], 'topo_weight': [], 'G': 1})
        assert e.value.code == -6
    a.sweep(1)
    with pytest.raises(_ffi.PhyloError) as e:               # a sweep but no summary of it
        a.tree_branches({'clade_weight': [], 'topo_weight': [], 'G': 1})
    assert e.value.code == -6
    ta = a.tree_summary()
    first = a.tree_branches(ta)
    again = a.tree_branches(ta)                             # repeatable
    ta2 = a.tree_summary()                                  # ... and the summary's tables are what they were
    b.sweep(1)
    tb = b.tree_summary()
    for key in ('clade_bits', 'clade_weight', 'clade_group', 'topo_weight', 'topo_count', 'topo_rep', 'topo_group', 'particle_topo',
                'u', 'U'):
        np.testing.assert_array_equal(ta[key], tb[key], err_msg=key)
        np.testing.assert_array_equal(ta2[key], tb[key], err_msg=key)
    for key in STATS:
        np.testing.assert_array_equal(first[key], again[key], err_msg=key)
    ra, rb = a.sweep(2), b.sweep(2)                         # the next sweep's bits: b never ran the branch pass
    for key in ('log_weights', 'log_likelihood', 'left_branches', 'right_branches'):
        assert np.array_equal(ra[key].view(np.uint64), rb[key].view(np.uint64)), key
    assert np.array_equal(ra['ancestors'], rb['ancestors']) and ra['logZ'] == rb['logZ']
    with pytest.raises(_ffi.PhyloError) as e:               # the newer sweep made the summary stale
        a.tree_branches(ta)
    assert e.value.code == -6
    a.close()
    b.close()


def test_vcsmc_branch_lengths_against_the_particle_newicks():
    d = synthetic_alignment(16, 60, seed=76)                # ends on several topologies, some of them of one weighted particle
    v = VCSMC(d, K=256, args=default_args(jcmodel=True, seed=1))
    v.sample_phylogenies()
    plain = v.tree_posterior()
    post = v.tree_posterior(branch_lengths=True)
    assert not hasattr(plain, 'consensus_bl') and plain.to_json() == post.to_json()
    N, seen = v.N, 0
    for t in post.topologies:
        if t['count'] != 1 or t['weight'] == 0:
            continue
        # a topology of one particle: its conditional means are that particle's own lengths (one rounding of u b / u)
        mine = TP.tree_newick(v.taxa, [(post.clade_sets[j][0], m) for j, m in zip(t['clades'], t['clade_means'])], t['leaf_means'])
        a, b = TP.newick_branches(mine, v.taxa), TP.newick_branches(v.newick(t['representative']), v.taxa)
        assert a.keys() == b.keys() and len(a) == 2 * N - 2
        for key in a:
            assert '%.6g' % a[key] == '%.6g' % b[key], (key, a[key], b[key])
        seen += 1
    assert seen > 0
    got = TP.newick_branches(post.consensus_bl, v.taxa)
    for j, (m, s) in enumerate(post.clade_sets):
        if s > 0.5:
            assert '%.6g' % got[m] == '%.6g' % post.clade_branches[j]['mean']
    assert TP.newick_clades(post.consensus_bl, v.taxa) == TP.newick_clades(post.consensus, v.taxa)
    assert TP.newick_clades(post.map_newick, v.taxa) == {post.clade_sets[j][0] for j in post.map['clades']}
    assert set(post.leaf_branches) == set(str(x) for x in v.taxa)
    v.close()


def run_world(world, K, dataset, seed, keep):
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, PHYLO_RDZV_DIR=tmp, MASTER_PORT=str(29300 + os.getpid() % 600 + world), PHYLO_COMM='hostshm')
        procs = []
        for r in range(world):
            out = os.path.join(tmp, "r%d.npz" % r)
            procs.append((out, subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_tree_branches_worker.py"), str(r),
                                                 str(world), str(K), dataset, str(seed), str(int(keep)), out],
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


@pytest.mark.parametrize("world,K,keep", [(2, 64, False), (3, 96, False), (2, 64, True)])
def test_sharded_ranks_return_the_unsharded_tables(world, K, keep):
    g = load_dataset('primate_data_wang')['genome']
    ctx = make_ctx(g, K)
    ctx.sweep(4)
    one = both(ctx)
    ctx.close()
    for t in run_world(world, K, 'primate_data_wang', 4, keep):
        for key in ('clade_bits', 'clade_weight', 'topo_weight', 'particle_topo', 'u') + STATS:
            a, b = t[key], one[key]
            if a.dtype == np.float64:
                a, b = a.view(np.uint64), b.view(np.uint64)
            np.testing.assert_array_equal(a, b, err_msg=key)


def test_runner_tree_branches_writes_three_more_files():
    argv = ['--dataset', 'primate_data_wang', '--n_particles', '16', '--num_epoch', '0', '--jcmodel', 'true', '--seed', '2']   # (no training:
    # the minibatch draws are unseeded, the evaluation sweep is not)
    seen = {}
    for name, extra in (('summary', ['--tree_summary', 'true']), ('both', ['--tree_summary', 'true', '--tree_branches', 'true'])):
        with tempfile.TemporaryDirectory() as tmp:
            p = subprocess.run([sys.executable, os.path.join(ROOT, 'runner.py')] + argv + extra, cwd=tmp,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
            assert p.returncode == 0, p.stdout.decode()[-2000:]
            (res,) = glob.glob(os.path.join(tmp, 'results', '*', '*', '*', '*', 'results.p'))
            d = os.path.dirname(res)
            files = {}
            for f in sorted(os.listdir(d)):
                with open(os.path.join(d, f), 'rb') as h:
                    files[f] = h.read()
            with open(res, 'rb') as f:
                files['keys'] = sorted(pickle.load(f))
            seen[name] = files
    today = ['consensus.tre', 'keys', 'results.p', 'run_parameters.txt', 'tree_posterior.json']
    assert sorted(seen['summary']) == today
    assert sorted(seen['both']) == sorted(today + ['consensus_bl.tre', 'map.tre', 'tree_branches.json'])
    for f in ('consensus.tre', 'tree_posterior.json', 'keys'):           # the same seeded run: byte for byte
        assert seen['summary'][f] == seen['both'][f], f
    taxa = load_dataset('primate_data_wang')['taxa']
    cons = TP.newick_branches(seen['both']['consensus_bl.tre'].decode().strip(), taxa)
    assert TP.newick_clades(seen['both']['consensus_bl.tre'].decode().strip(), taxa) == \
        TP.newick_clades(seen['both']['consensus.tre'].decode().strip(), taxa)
    assert all(i in cons for i in range(len(taxa)))
    assert len(TP.newick_branches(seen['both']['map.tre'].decode().strip(), taxa)) == 2 * len(taxa) - 2
