"""Host side of the tree posterior's branch lengths (phylo_amd/treepost.py) on hand-made tables: means from the device's sums,
the consensus and MAP Newick with lengths read back through newick_branches, "no estimate" for a weight of 0, the runner flag,
and the files of a run without the flag.  CPU only; the device tables are covered by tests/test_gpu_tree_branches.py."""
import json
import os
import tempfile

import numpy as np
import pytest

from phylo_amd import treepost as TP

TAXA = ['A', 'B', 'C', 'D', 'E']


def sums(weight, mean, spread=0.0):
    """a (S1, S2, min, max) row whose mean over `weight` is `mean`"""
    return [weight * mean, weight * (mean * mean + spread * spread), mean - spread, mean + spread]


def table():
    """two topologies over five taxa, U = 8: ((A,B),((C,D),E)) with weight 6 and ((A,B),(C,(D,E))) with weight 2"""
    clades = [((0, 1), 8), ((2, 3, 4), 8), ((2, 3), 6), ((3, 4), 2)]
    bits = np.array([[sum(1 << i for i in m)] for m, _ in clades], dtype=np.uint64)
    cmeans = [0.5, 0.25, 0.125, 2.0]
    lmeans = [0.1, 0.2, 0.3, 0.4, 0.6]
    return {'clade_bits': bits, 'clade_weight': np.array([w for _, w in clades], dtype=np.uint64),
            'topo_weight': np.array([6, 2], dtype=np.uint64), 'topo_count': np.array([3, 1], dtype=np.int32),
            'topo_rep': np.array([0, 2], dtype=np.int32), 'particle_topo': np.array([0, 0, 1, 0], dtype=np.int32), 'U': 8,
            'clade_stats': np.array([sums(w, m, 0.0625) for (_, w), m in zip(clades, cmeans)]),
            'leaf_stats': np.array([sums(8, m) for m in lmeans]),
            'topo_clades': np.array([[0, 1, 2], [0, 1, 3]], dtype=np.int32),
            'topo_stats': np.array([[sums(6, m) for m in lmeans] + [sums(6, m) for m in (0.75, 0.5, 0.125)],
                                    [sums(2, m) for m in lmeans] + [sums(2, m) for m in (1.5, 1.0, 2.0)]])}, cmeans, lmeans


def summary_only(tab):
    return {k: v for k, v in tab.items() if k not in ('clade_stats', 'leaf_stats', 'topo_clades', 'topo_stats')}


def test_consensus_and_map_newick_read_back_to_the_tables_means():
    tab, cmeans, lmeans = table()
    post = TP.TreePosterior(TAXA, tab, newicks={0: 'x;', 2: 'y;'})
    assert [b['mean'] for b in post.clade_branches] == cmeans
    assert post.clade_branches[0]['sd'] == pytest.approx(0.0625) and post.clade_branches[0]['min'] == 0.5 - 0.0625
    assert post.leaf_branches['E']['mean'] == 0.6
    got = TP.newick_branches(post.consensus_bl, TAXA)
    want = {frozenset({0, 1}): 0.5, frozenset({2, 3, 4}): 0.25, frozenset({2, 3}): 0.125}        # support 0.75 > 0.5; (D,E) is out
    want.update({i: m for i, m in enumerate(lmeans)})
    assert got == want
    assert TP.newick_clades(post.consensus_bl, TAXA) == TP.newick_clades(post.consensus, TAXA)
    assert post.consensus_bl == '((A:0.1,B:0.2)1:0.5,((C:0.3,D:0.4)0.75:0.125,E:0.6)1:0.25);'
    # the MAP topology from topo_clades and ITS conditional means, no representative particle
    assert post.topologies[0]['clades'] == [0, 1, 2] and post.topologies[1]['clade_means'] == [1.5, 1.0, 2.0]
    got = TP.newick_branches(post.map_newick, TAXA)
    assert got == {frozenset({0, 1}): 0.75, frozenset({2, 3, 4}): 0.5, frozenset({2, 3}): 0.125, **dict(enumerate(lmeans))}
    assert post.map_newick == '((A:0.1,B:0.2):0.75,((C:0.3,D:0.4):0.125,E:0.6):0.5);'


def test_weight_zero_renders_no_length():
    tab, _, _ = table()
    tab['clade_weight'][3] = 0                                   # (D,E) held only by particles of integer weight 0 ...
    tab['clade_stats'][3] = [0.0, 0.0, 2.0, 2.0]
    tab['topo_weight'][1] = 0                                    # ... which are all of topology 1
    tab['topo_stats'][1, :, :2] = 0.0
    post = TP.TreePosterior(TAXA, tab)
    assert post.clade_branches[3] == {'mean': None, 'sd': None, 'min': 2.0, 'max': 2.0}
    assert post.topologies[1]['clade_means'] == [None, None, None] and post.topologies[1]['leaf_means'] == [None] * 5
    one = dict(tab, topo_weight=tab['topo_weight'][1:], topo_count=tab['topo_count'][1:], topo_rep=tab['topo_rep'][1:],
               topo_clades=tab['topo_clades'][1:], topo_stats=tab['topo_stats'][1:])
    s = TP.TreePosterior(TAXA, one).map_newick                   # a MAP topology of weight 0: a cladogram, no NaN in the file
    assert s == '((A,B),(C,(D,E)));' and TP.newick_branches(s, TAXA) == {}
    lone = TP.tree_newick(TAXA, [(frozenset({3, 4}), None)], [0.5, None, 0.5, 0.5, 0.5])   # an edge without an estimate
    assert lone == '(A:0.5,B,C:0.5,(D:0.5,E:0.5));' and frozenset({3, 4}) not in TP.newick_branches(lone, TAXA)
    assert 'nan' not in post.consensus_bl.lower()
    text = json.dumps(post.branches_json())                      # None, not NaN
    assert 'NaN' not in text and json.loads(text)['clades'][3]['mean'] is None


def test_newick_branches_reader():
    s = '((A:0.1,B:0.2)0.9:0.3,(C:1,(D:2e-3,E)0.7):0.5);'
    assert TP.newick_branches(s, TAXA) == {0: 0.1, 1: 0.2, frozenset({0, 1}): 0.3, 2: 1.0, 3: 0.002, frozenset({2, 3, 4}): 0.5}
    with pytest.raises(ValueError):
        TP.newick_branches('((A:1,B:1):1,X:1);', TAXA)


def test_group_table_carries_the_branch_slices():
    tab, _, _ = table()
    full = dict(summary_only(tab), G=1, u=np.ones(4, dtype=np.uint64), U=np.array([8], dtype=np.uint64),
                clade_offsets=np.array([0, 4]), topo_offsets=np.array([0, 2]))
    assert 'clade_stats' not in TP.group_table(full, 0)
    full.update(clade_stats=tab['clade_stats'], leaf_stats=tab['leaf_stats'][None], topo_clades=tab['topo_clades'],
                topo_stats=tab['topo_stats'])
    g = TP.group_table(full, 0)
    assert g['leaf_stats'].shape == (5, 4) and g['topo_stats'].shape == (2, 8, 4) and g['clade_stats'].shape == (4, 4)


def test_default_posterior_and_its_files_do_not_change():
    tab, _, _ = table()
    newicks = {0: '((A:1,B:1):1,((C:1,D:1):1,E:1):1);', 2: '((A:1,B:1):1,(C:1,(D:1,E:1):1):1);'}
    plain, rich = TP.TreePosterior(TAXA, summary_only(tab), newicks), TP.TreePosterior(TAXA, tab, newicks)
    assert not hasattr(plain, 'consensus_bl') and not hasattr(plain, 'clade_branches') and 'clades' not in plain.topologies[0]
    assert sorted(plain.to_json()) == ['clades', 'consensus', 'map', 'taxa', 'threshold', 'topologies', 'total_weight']
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        plain.write(a)
        rich.write(b)
        rich.write_branches(b)
        assert sorted(os.listdir(a)) == ['consensus.tre', 'tree_posterior.json']
        assert sorted(os.listdir(b)) == ['consensus.tre', 'consensus_bl.tre', 'map.tre', 'tree_branches.json', 'tree_posterior.json']
        for name in os.listdir(a):                               # the summary's two files, byte for byte
            with open(os.path.join(a, name), 'rb') as f, open(os.path.join(b, name), 'rb') as h:
                assert f.read() == h.read(), name
        with open(os.path.join(b, 'map.tre')) as f:
            assert f.read() == rich.map_newick + '\n'


def test_tree_branches_flag_needs_tree_summary():
    import runner
    assert runner.parse_args([]).tree_branches is False
    assert runner.parse_args(['--tree_summary', 'true']).tree_branches is False
    a = runner.parse_args(['--tree_summary', 'true', '--tree_branches', 'true'])
    assert a.tree_summary is True and a.tree_branches is True
    for argv in (['--tree_branches', 'true'], ['--tree_branches', 'true', '--tree_summary', 'false']):
        with pytest.raises(SystemExit):
            runner.parse_args(argv)


def test_run_parameters_file_is_unchanged_with_the_flag_off():
    import runner
    from phylo_amd.datasets import synthetic_alignment
    from phylo_amd.vcsmc import VCSMC
    hist = {k: [] for k in ('cost', 'log_weights', 'Qmatrices', 'left_branches', 'right_branches', 'log_lik', 'll_tilde',
                            'log_lik_R', 'jump_chain_evolution', 'newick')}
    texts = []
    for strip in (False, True):
        args = runner.parse_args(['--jcmodel', 'true'])
        if strip:
            del args.tree_branches                               # the namespace of the parser before the flag existed
        v = VCSMC(synthetic_alignment(4, 8, seed=1), K=4, args=args)
        v.lr = 0.001
        with tempfile.TemporaryDirectory() as tmp:
            v._save_results(tmp, 0.0, hist)
            assert sorted(os.listdir(tmp)) == ['results.p', 'run_parameters.txt']
            with open(os.path.join(tmp, 'run_parameters.txt'), 'rb') as f:
                texts.append(f.read())
    assert texts[0] == texts[1] and b'tree_summary' in texts[0] and b'tree_branches' not in texts[0]
