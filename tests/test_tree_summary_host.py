"""Host side of the tree posterior summary (phylo_amd/treepost.py) on hand-made clade tables: the majority-rule consensus, its
Newick, credible sets, and the runner flag.  CPU only; the device tables are covered by tests/test_gpu_tree_summary.py."""
import numpy as np
import pytest

from phylo_amd import treepost as TP

TAXA = ['A', 'B', 'C', 'D', 'E']


def table(clades, topos, U, K=None):
    """a group table in the layout of Context.tree_summary(): clades = [(taxon indices, weight)], topos = [(weight, count, rep)]"""
    bits = np.array([[sum(1 << i for i in m)] for m, _ in clades], dtype=np.uint64).reshape(-1, 1)
    return {'clade_bits': bits, 'clade_weight': np.array([w for _, w in clades], dtype=np.uint64),
            'topo_weight': np.array([t[0] for t in topos], dtype=np.uint64), 'topo_count': np.array([t[1] for t in topos], dtype=np.int32),
            'topo_rep': np.array([t[2] for t in topos], dtype=np.int32), 'particle_topo': np.zeros(K or 1, dtype=np.int32), 'U': U}


def test_nothing_above_threshold_gives_a_star():
    assert TP.consensus_newick(TAXA, [({0, 1}, 0.5), ({2, 3}, 0.3)]) == '(A,B,C,D,E);'
    assert TP.newick_clades('(A,B,C,D,E);', TAXA) == set()


def test_one_topology_with_all_the_weight_gives_that_tree():
    # ((A,B),((C,D),E)) holds every particle: its three non-trivial clades have support 1
    post = TP.TreePosterior(TAXA, table([((0, 1), 8), ((2, 3), 8), ((2, 3, 4), 8)], [(8, 4, 0)], 8, K=4),
                            newicks={0: '((A:1,B:1):1,((C:1,D:1):1,E:1):1);'})
    assert post.consensus == '((A,B)1,((C,D)1,E)1);'
    assert TP.newick_clades(post.consensus, TAXA) == {frozenset({0, 1}), frozenset({2, 3}), frozenset({2, 3, 4})}
    assert TP.newick_clades(post.map['newick'], TAXA) == TP.newick_clades(post.consensus, TAXA)
    assert post.map['probability'] == 1.0 and post.map['count'] == 4
    assert post.clades[2] == (('C', 'D', 'E'), 1.0)


def test_a_clade_at_exactly_one_half_is_excluded():
    clades = [((0, 1), 3), ((2, 3), 2), ((0, 1, 2), 1)]
    post = TP.TreePosterior(TAXA, table(clades, [(2, 1, 0), (1, 1, 1), (1, 1, 2)], 4, K=3))
    assert [s for _, s in post.clades] == [0.75, 0.5, 0.25]
    assert post.consensus == '((A,B)0.75,C,D,E);'
    assert TP.consensus_newick(TAXA, post.clade_sets, threshold=0.4) == '((A,B)0.75,(C,D)0.5,E);'


def test_incompatible_clades_below_one_half_are_refused():
    with pytest.raises(ValueError):
        TP.consensus_newick(TAXA, [({0, 1}, 0.45), ({1, 2}, 0.45)], threshold=0.3)


def test_credible_set_order_and_ties():
    # table order (weight descending, ties by representative) is the device's; credible_set takes its shortest prefix
    post = TP.TreePosterior(TAXA, table([], [(5, 2, 3), (3, 1, 0), (3, 1, 4), (1, 1, 1)], 12, K=5))
    reps = lambda ts: [t['representative'] for t in ts]
    assert reps(post.credible_set(0.0)) == [3]
    assert reps(post.credible_set(5 / 12)) == [3]
    assert reps(post.credible_set(0.5)) == [3, 0]
    assert reps(post.credible_set(8 / 12)) == [3, 0]
    assert reps(post.credible_set(0.9)) == [3, 0, 4]
    assert reps(post.credible_set(0.95)) == [3, 0, 4, 1]
    assert reps(post.credible_set(1.0)) == [3, 0, 4, 1]
    assert post.map['representative'] == 3
    with pytest.raises(ValueError):
        post.credible_set(1.5)


def test_newick_reader_skips_lengths_and_labels():
    s = '((A:0.1,B:0.2)0.9:0.3,(C:1,(D:2,E:3)0.7:1):0.5);'
    assert TP.newick_clades(s, TAXA) == {frozenset({0, 1}), frozenset({2, 3, 4}), frozenset({3, 4})}
    with pytest.raises(ValueError):
        TP.newick_clades('((A,B),X);', TAXA)


def test_bits_to_indices_across_words():
    row = np.array([1 << 63, 5], dtype=np.uint64)
    assert TP.bits_to_indices(row) == [63, 64, 66]


def test_tree_summary_flag_defaults_to_false():
    import runner
    assert runner.parse_args([]).tree_summary is False
    assert runner.parse_args(['--tree_summary', 'true']).tree_summary is True
    assert runner.parse_args(['--tree_summary', 'false']).tree_summary is False
