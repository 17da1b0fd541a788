"""Marginal ancestral state posteriors without a GPU: the NumPy restatement of phylo_trees_ancestral's
contract (treeanc_ref.py) against an enumeration of every assignment of internal states and against the same formulas at 50
digits (E_REF_ANC, from which the device tolerance follows); its row sums; the host half of phylo_treeanc.h under sanitizers;
phylo_amd.ancestral on hand-made arrays; the runner's parser errors.

Every test here fails without the feature: on import of phylo_amd.ancestral, or on the missing symbol, header or flag."""
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import treeanc_cases as AC
import treeanc_ref as AR
from oracle import cpu_ref as O
from phylo_amd import _ffi
from phylo_amd import ancestral as A
from treeanc_cases import E_REF_ANC, SUM_ERR, SUM_TOL, TOL_ANC, gapped
from treegrad_cases import branch_matrices
from trees_cases import random_rows

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PRIOR = np.array([0.1, 0.2, 0.3, 0.4])


# ---- (a) -----------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported():
    assert 'phylo_trees_ancestral' in _ffi.EXPORTS
    assert _ffi.ANC_NOSTATE == A.NOSTATE == AR.NOSTATE == 255
    with open(os.path.join(ROOT, 'include', 'phylo_hip.h')) as f:
        head = f.read()
    assert '#define PHYLO_ANC_NOSTATE 255' in head and 'int phylo_trees_ancestral(' in head


# ---- (b) the restatement computes marginals: every assignment of internal states enumerated -------------------------------------
def enumerated(child, M, prior, g):
    """post [N-1][S][4] and L [S] by summing prior[root] prod_b M_b[child state][parent state] (a leaf: its row . M_b[:, parent
    state]) over all 4^(N-1) assignments of the internal states -- no recursion, no messages"""
    R = child.shape[0]
    N, S = R + 1, g.shape[1]
    num = np.zeros((R, S, 4))
    for z in itertools.product(range(4), repeat=R):
        w = np.full(S, prior[z[R - 1]])
        for i in range(R):
            for sd in range(2):
                ch = child[i, sd]
                w = w * (g[ch] @ M[i, sd][:, z[i]] if ch < N else M[i, sd][z[ch - N], z[i]])
        for i in range(R):
            num[i, :, z[i]] += w
    L = num[R - 1].sum(axis=1)
    return num / L[None, :, None], L


@pytest.mark.parametrize("N", [3, 4, 5])
@pytest.mark.parametrize("jc", [False, True], ids=['gtr', 'jc'])
def test_reference_computes_marginals(N, jc):
    S = 6
    rng = np.random.default_rng(10 * N + jc)
    g = gapped(N, S, rng)
    g[1] = rng.uniform(0.05, 1.0, size=(S, 4))             # one generic row
    Q = O.jc_Q() if jc else O.get_Q(rng.normal(size=(4, 4)))
    worst = 0.0
    for _ in range(4):
        child, blen = random_rows(N, rng)
        M = branch_matrices(Q, blen)
        _, post, state, pmax, L = AR.tree_ancestral(child, M, PRIOR, g)
        want, Le = enumerated(child, M, PRIOR, g)
        np.testing.assert_allclose(L, Le, rtol=1e-13, atol=0)
        np.testing.assert_allclose(post, want, rtol=1e-13, atol=1e-300)
        worst = max(worst, float(np.max(np.abs(post - want) / np.maximum(want, 1e-300))))
        np.testing.assert_array_equal(state, np.argmax(post, axis=-1))
        np.testing.assert_array_equal(pmax, post.max(axis=-1))
    print("restatement against the enumeration: worst relative difference %.3g" % worst)


# ---- (c), (d) the same formulas at 50 digits: E_REF_ANC; the row sums -------------------------------------------------------------
def mp_cases():
    N, S = 5, 8
    for seed in range(20):
        for jc in (False, True):
            rng = np.random.default_rng(seed)
            g = gapped(N, S, rng)
            Q = O.jc_Q() if jc else O.get_Q(rng.normal(size=(4, 4)))
            child, blen = random_rows(N, rng)
            yield child, branch_matrices(Q, blen), g


def test_reference_against_mpmath():
    """N = 5, S = 8, gaps; 20 random trees under a GTR-like Q and under JC69 (section 13's recipe).  The worst |reference -
    50-digit value| over every posterior, in units of |value| 2^-53 (every term is non-negative: nothing cancels), is
    E_REF_ANC: the restatement's own error, from which TOL_ANC = 8 E_REF_ANC 2^-53 follows.  Measured here: 7.17."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    mpf = mp.mpf
    worst = 0.0
    for child, M, g in mp_cases():
        N, S = g.shape[0], g.shape[1]
        post = AR.tree_ancestral(child, M, PRIOR, g)[1]
        Mm = [[[[mpf(float(v)) for v in r] for r in M[i, sd]] for sd in range(2)] for i in range(N - 1)]
        pm = [mpf(float(v)) for v in PRIOR]
        for s in range(S):
            rows = [[mpf(float(v)) for v in g[i, s]] for i in range(N)]
            _, exact = AR.site_terms(child.tolist(), Mm, pm, rows, mpf(0))
            for i in range(N - 1):
                for j in range(4):
                    if exact[i][j] == 0:
                        assert post[i, s, j] == 0.0
                    else:
                        worst = max(worst, float(abs(mpf(float(post[i, s, j])) - exact[i][j]) / (abs(exact[i][j]) * mpf(2) ** -53)))
    print("reference against 50 digits: worst error %.3f units of |value| 2^-53 (E_REF_ANC = %g, TOL_ANC = %.3g)" % (worst, E_REF_ANC, TOL_ANC))
    assert E_REF_ANC / 2 <= worst <= E_REF_ANC


def test_reference_posteriors_sum_to_one():
    """post is not renormalised: |sum_j post_j - 1| of the restatement over the cases of (c) is at most SUM_ERR = 6 * 2^-53,
    measured here; held at 8 times that"""
    worst = 0.0
    for child, M, g in mp_cases():
        post = AR.tree_ancestral(child, M, PRIOR, g)[1]
        worst = max(worst, float(np.abs(post.sum(axis=-1) - 1.0).max()))
    print("worst |sum_j post_j - 1| = %.3g = %.2f * 2^-53 (SUM_ERR %.3g, held at %.3g)" % (worst, worst * 2.0 ** 53, SUM_ERR, SUM_TOL))
    assert worst <= SUM_TOL


def test_reference_nan_rule_is_per_site():
    """a site whose factor lies below the floor is NaN / NOSTATE in its own column at every node; every other column keeps its bits"""
    rng = np.random.default_rng(5)
    N, S = 5, 6
    g = gapped(N, S, rng)
    child, blen = random_rows(N, rng)
    M = branch_matrices(O.get_Q(rng.normal(size=(4, 4))), blen)
    _, post, state, pmax, L = AR.tree_ancestral(child, M, PRIOR, g)
    g2 = g.copy()
    g2[0, 3] *= 2.0 ** -1021                                # scales that site's factor below 2^-1020
    g2[1, 4] = 0.0                                         # and one site has no likelihood at all
    _, post2, state2, pmax2, L2 = AR.tree_ancestral(child, M, PRIOR, g2)
    assert 0 < L2[3] < AR.FLOOR and L2[4] == 0.0
    assert np.isnan(post2[:, 3:5]).all() and (state2[:, 3:5] == AR.NOSTATE).all() and np.isnan(pmax2[:, 3:5]).all()
    keep = [0, 1, 2, 5]
    np.testing.assert_array_equal(post2[:, keep].view(np.uint64), post[:, keep].view(np.uint64))
    np.testing.assert_array_equal(state2[:, keep], state[:, keep])


def test_device_cases_decide_their_states():
    """the precondition of the device test's comparison of states: in every case of test_gpu_trees_loglik.CASES the restatement's
    two largest posteriors differ by more than 2 TOL_ANC relative at more than 99 % of the node-sites (scipy's matrices here, the
    device's own there, where it is asserted again)"""
    from test_gpu_trees_loglik import CASES
    for name in CASES:
        g, Q, child, blen, jc, n, tile = AC.case_inputs(name)
        post = AR.trees_ancestral(child, branch_matrices(Q, blen), AC.PRIOR, g)[1]
        assert np.isfinite(post).all(), name
        share = 1.0 - AC.decided(post).mean()
        print("%s: %.4f %% of the node-sites undecided" % (name, 100 * share))
        assert share < AC.MAX_EXCLUDED, (name, share)
        assert np.abs(post.sum(axis=-1) - 1.0).max() < 1e-12, name


# ---- (e) the host half under sanitizers ------------------------------------------------------------------------------------------
def test_header_under_sanitizers(tmp_path):
    """The host half of phylo_treeanc.h with a main of its own (tests/treeanc_asan_main.cpp), address and undefined-behaviour
    sanitizers of the host compiler: output-bound chunks, the growth to one tree over 256 MiB, the refusal above 1 GiB."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "treeanc_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "phylo_amd", "csrc"), os.path.join(ROOT, "tests", "treeanc_asan_main.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    assert b"0 values differ" in p.stdout


# ---- (f) phylo_amd.ancestral on hand-made arrays ----------------------------------------------------------------------------------
def test_map_states_ties_and_nostate():
    nan = np.nan
    post = np.array([[0.1, 0.4, 0.4, 0.1],                 # a tie: the lowest index
                     [0.25, 0.25, 0.25, 0.25],
                     [0.0, 0.0, 0.0, 1.0],
                     [0.7, nan, 0.2, 0.1],                 # any NaN: no state
                     [nan, nan, nan, nan],
                     [0.0, 0.0, 0.0, 0.0]])
    state, pmax = AR.map_states(post)
    np.testing.assert_array_equal(state, [1, 0, 3, 255, 255, 0])
    np.testing.assert_array_equal(pmax, [0.4, 0.25, 1.0, nan, nan, 0.0])
    assert state.dtype == np.uint8
    assert A.sequences(state[None]) == ['CAT??A']


def test_sequences_and_fasta_round_trip(tmp_path):
    state = np.array([[0, 1, 2, 3, 255], [3, 3, 255, 0, 0]], dtype=np.uint8)
    assert A.sequences(state) == ['ACGT?', 'TT?AA']
    assert A.sequences(state, letters='acgu', nostate='-') == ['acgu-', 'uu-aa']
    with pytest.raises(ValueError):
        A.sequences(np.array([[4]], dtype=np.uint8))
    with pytest.raises(ValueError):
        A.sequences(state, letters='ACG')
    child = np.array([[0, 1], [3, 2]])
    recs = A.fasta_records(state, child, ['x', 'y', 'w'], tree=4)
    assert recs == [('tree4_node3 clade=x,y', 'ACGT?'), ('tree4_node4 clade=w,x,y', 'TT?AA')]
    for width in (0, 2):
        path = str(tmp_path / ('a%d.fa' % width))
        A.write_fasta(path, recs, width=width)
        assert A.read_fasta(path) == recs
    with open(str(tmp_path / 'a0.fa')) as f:
        assert f.read() == '>tree4_node3 clade=x,y\nACGT?\n>tree4_node4 clade=w,x,y\nTT?AA\n'


def test_node_clades_of_a_caterpillar_and_a_balanced_tree():
    taxa = ['e', 'd', 'c', 'b', 'a']
    cat = np.array([[0, 1], [5, 2], [6, 3], [4, 7]])
    assert A.node_clades(cat, taxa) == [['d', 'e'], ['c', 'd', 'e'], ['b', 'c', 'd', 'e'], ['a', 'b', 'c', 'd', 'e']]
    taxa8 = list('hgfedcba')
    bal = np.array([[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10, 11], [12, 13]])
    assert A.node_clades(bal, taxa8) == [['g', 'h'], ['e', 'f'], ['c', 'd'], ['a', 'b'], ['e', 'f', 'g', 'h'], ['a', 'b', 'c', 'd'],
                                         list('abcdefgh')]
    with pytest.raises(ValueError):
        A.node_clades(np.array([[0, 4], [1, 2]]), ['a', 'b', 'c'])      # a child from a later row
    with pytest.raises(ValueError):
        A.node_clades(cat, taxa[:4])


def test_summarise_excludes_and_counts_nan_sites():
    nan = np.nan
    pmax = np.array([[1.0, 0.5, 0.9, nan],
                     [0.89, 0.89, nan, nan],
                     [nan, nan, nan, nan]])
    sm = A.summarise(pmax)
    np.testing.assert_array_equal(sm['n_nan'], [1, 2, 4])
    np.testing.assert_allclose(sm['mean_pmax'][:2], [0.8, 0.89])
    np.testing.assert_allclose(sm['share_below'][:2], [1 / 3, 1.0])          # 0.9 itself is not below 0.9
    assert np.isnan(sm['mean_pmax'][2]) and np.isnan(sm['share_below'][2])


# ---- (g) the runner's parser --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,what", [
    (['--score_ancestral', '2'], '--score_ancestral needs --score_trees'),
    (['--score_ancestral', '0', '--score_trees', 'x.nwk'], 'K >= 1'),
    (['--score_ancestral', '2', '--score_trees', 'x.nwk', '--score_rates', 'gamma:0.5:4'], 'not built for rate mixtures'),
    (['--score_ancestral', '2', '--score_trees', 'x.nwk', '--score_rates', 'gamma:0.5:4', '--score_fit', 'branches'],
     'not built for rate mixtures'),
    (['--score_ancestral', '2', '--score_trees', 'x.nwk', '--score_rates', 'gamma:0.5:4', '--score_fit', 'branches',
      '--score_fit_search', 'nni'], 'not built for rate mixtures'),
])
def test_runner_parser_errors(argv, what, capsys):
    sys.path.insert(0, ROOT)
    try:
        import runner
    finally:
        sys.path.remove(ROOT)
    with pytest.raises(SystemExit) as e:
        runner.parse_args(['--dataset', 'primate_data_wang'] + argv)
    assert e.value.code == 2 and what in capsys.readouterr().err
    base = ['--dataset', 'primate_data_wang', '--score_trees', 'x.nwk', '--score_ancestral', '3']
    assert runner.parse_args(base).score_ancestral == 3
    assert runner.parse_args(base + ['--score_opt', 'true', '--score_search', 'nni']).score_ancestral == 3
    assert runner.parse_args(base + ['--score_opt', 'true', '--score_model_fit', 'q']).score_ancestral == 3
    assert runner.parse_args(['--dataset', 'primate_data_wang']).score_ancestral is None
