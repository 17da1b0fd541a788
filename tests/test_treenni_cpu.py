"""NNI neighbourhoods and NNI search without a GPU: the NumPy restatement of phylo_trees_nni's contract
(treenni_ref.py) against the same formulas at 50 digits and against the restated log-likelihood of every explicitly built
neighbour; phylo_amd.treesearch's moves as rows; nni_search driven by the restatements; the runner's parser; the host half of
phylo_treenni.h under sanitizers.

Every test here fails on import without phylo_amd.treesearch."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import treenni_cases as NC
import treenni_ref as NR
from phylo_amd import _ffi
from phylo_amd.treesearch import apply_nni, nni_moves, nni_search
from treegrad_cases import branch_matrices
from trees_cases import random_rows

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_symbol_is_exported():
    assert 'phylo_trees_nni' in _ffi.EXPORTS


# ---- (a) the restatement at 50 digits, and against explicit neighbours: E_NNI, E_EXPL -----------------------------------------
def test_reference_against_mpmath():
    """Every move of the trees of treenni_cases.small_cases.  E_NNI: the worst |restated delta - 50-digit delta| in units of
    (S + sum_s |d_s|) 2^-53 (a relative error of L'_s is an absolute error of its log: the S term).  E_EXPL: for loglik + delta
    against the restated log-likelihood of apply_nni's tree, the errors of both sides against the 50-digit log-likelihood of that
    tree, added, in units of (S + sum_s |log L_s| + sum_s |log L'_s|) 2^-53.  The 50-digit value of the move and of the explicit
    neighbour agree to 40 digits: the move IS that tree.  Measured here: 2.86 and 1.60."""
    mp = pytest.importorskip("mpmath")
    worst_n = worst_x = 0.0
    seen = 0
    for name, child, blen, Q, g in NC.small_cases():
        S = g.shape[1]
        M = branch_matrices(Q, blen)
        ll, delta, absd = NR.tree_nni(child, M, NC.PRIOR, g)
        ell, eal, emv = NC.mp_tree(mp, child, M, NC.PRIOR, g)
        assert set(emv) == set(nni_moves(child)), name
        assert np.isnan(delta).sum() == delta.size - len(emv), name
        for (r, sd), (ed, ea, dead) in emv.items():
            seen += 1
            if dead:                                                      # an impossible neighbour (zero-length branches)
                assert delta[r, sd] == -np.inf, (name, r, sd)
                continue
            err = float(abs(mp.mpf(float(delta[r, sd])) - ed) / ((S + ea) * mp.mpf(2) ** -53))
            assert abs(float(ea) - absd[r, sd]) <= 1e-9 * (1 + absd[r, sd])
            worst_n = max(worst_n, err)
            c2, b2 = apply_nni(child, blen, r, sd)
            M2 = branch_matrices(Q, b2)
            ll2, _ = NR.tree_loglik_sites(c2, M2, NC.PRIOR, g)
            ell2, eal2, _ = NC.mp_tree(mp, c2, M2, NC.PRIOR, g)
            assert abs(ell2 - (ell + ed)) < mp.mpf(10) ** -40, (name, r, sd)
            unit = (S + eal + eal2) * mp.mpf(2) ** -53
            both = float((abs(mp.mpf(float(ll + delta[r, sd])) - ell2) + abs(mp.mpf(ll2) - ell2)) / unit)
            worst_x = max(worst_x, both)
            assert abs((ll + delta[r, sd]) - ll2) <= NC.E_EXPL * float(unit), (name, r, sd)
    print("restatement against 50 digits over %d moves: delta %.3f units (E_NNI = %g), explicit neighbours %.3f units (E_EXPL = %g)"
          % (seen, worst_n, NC.E_NNI, worst_x, NC.E_EXPL))
    assert NC.E_NNI / 2 <= worst_n <= NC.E_NNI
    assert NC.E_EXPL / 2 <= worst_x <= NC.E_EXPL


# ---- (b) apply_nni and nni_moves ---------------------------------------------------------------------------------------------
def rows_ok(child, blen, N):
    R = N - 1
    assert child.shape == (R, 2) and blen.shape == (R, 2) and child.dtype == np.int32
    used = set()
    for i in range(R):
        for sd in range(2):
            ch = int(child[i, sd])
            assert 0 <= ch < N + i and ch not in used
            used.add(ch)
    assert used == set(range(2 * N - 2))


def subtree_lengths(child, blen):
    """{leaf set of a subtree: the length above it}"""
    R = child.shape[0]
    N = R + 1
    below = [frozenset([i]) for i in range(N)] + [None] * R
    out = {}
    for i in range(R):
        below[N + i] = below[child[i, 0]] | below[child[i, 1]]
        for sd in range(2):
            out[below[child[i, sd]]] = blen[i, sd]
    return out


@pytest.mark.parametrize("N", [3, 4, 5, 8, 12, 33])
def test_apply_nni(N):
    rng = np.random.default_rng(N)
    trees = [random_rows(N, rng, zeros=False) for _ in range(6)] + [make(N, rng) for make in NC.SHAPES.values()]
    if N in (3, 4):
        trees += [(c, rng.exponential(0.1, (N - 1, 2))) for c in NC.rooted_shapes(N)]
    for child, blen in trees:
        blen = blen + np.arange(2 * N - 2).reshape(N - 1, 2) * 1e-3       # every length its own
        R = N - 1
        moves = nni_moves(child)
        both = child[R - 1, 0] >= N and child[R - 1, 1] >= N
        assert len(moves) == 2 * (N - 2) + (2 if both else 0) and len(set(moves)) == len(moves)
        base = NC.clades(child)
        root_kids = {int(child[R - 1, 0]), int(child[R - 1, 1])}
        for row, side in moves:
            c2, b2 = apply_nni(child, blen, row, side)
            rows_ok(c2, b2, N)
            new = NC.clades(c2)
            changed = 0 if (row < R - 1 and N + row in root_kids) else 1    # a root-child move only shifts the root
            assert len(base - new) == changed and len(new - base) == changed, (row, side)
            old_len, new_len = subtree_lengths(child, blen), subtree_lengths(c2, b2)
            kept = set(old_len) & set(new_len)
            assert len(kept) >= 2 * N - 2 - 2 and all(old_len[k] == new_len[k] for k in kept)   # lengths travel with their subtrees
            assert sorted(b2.ravel()) == sorted(blen.ravel())
            assert any(NC.clades(apply_nni(c2, b2, *mv)[0]) == base for mv in nni_moves(c2))     # the inverse move
        for bad in [(R - 1, 0)] if not both else []:
            with pytest.raises(ValueError):
                apply_nni(child, blen, *bad)
        with pytest.raises(ValueError):
            apply_nni(child, blen, R, 0)


def test_child_order_is_the_contracts():
    child = np.array([[0, 1], [2, 3], [5, 6], [7, 4]], dtype=np.int32)       # N = 5: v = 5 = (0, 1), c = 6 = (2, 3), p = 7, root (7, 4)
    blen = np.arange(8, dtype=np.float64).reshape(4, 2) / 10
    c2, b2 = apply_nni(child, blen, 0, 0)                                    # y = 0, z = 1: v = (1, c), p = (v, 0)
    np.testing.assert_array_equal(c2, [[2, 3], [1, 5], [6, 0], [7, 4]])
    np.testing.assert_array_equal(b2, [[0.2, 0.3], [0.1, 0.5], [0.4, 0.0], [0.6, 0.7]])
    child = np.array([[0, 1], [2, 3], [5, 6], [4, 7]], dtype=np.int32)       # root (4, 7) has a leaf child: no move at the root
    assert (3, 0) not in nni_moves(child) and len(nni_moves(child)) == 6
    child = np.array([[0, 1], [2, 3], [5, 4], [7, 6]], dtype=np.int32)       # root = (v = 7 = (5, 4), c = 6 = (2, 3))
    c2, b2 = apply_nni(child, blen, 3, 1)                                    # b = 4 and c's side-1 child 3: v = (5, 3), c = (2, 4)
    np.testing.assert_array_equal(c2, [[0, 1], [5, 3], [2, 4], [6, 7]])
    np.testing.assert_array_equal(b2, [[0.0, 0.1], [0.4, 0.3], [0.2, 0.5], [0.6, 0.7]])


# ---- (c) the search --------------------------------------------------------------------------------------------------------------
def run_search(grad_fn, nni_fn, child, blen, eps=1e-6):
    """nni_search, with the margins of every decision: (result, least best - second-best delta of a taken move, least
    |best delta - eps|)"""
    marg = [np.inf, np.inf]

    def watched(c, b):
        ll, d = nni_fn(c, b)
        for x in np.asarray(d):
            f = np.sort(x[np.isfinite(x)])[::-1]
            marg[1] = min(marg[1], abs(f[0] - eps))
            if f[0] > eps:
                marg[0] = min(marg[0], f[0] - f[1])
        return ll, d

    return nni_search(grad_fn, watched, child, blen, max_rounds=10, eps=eps), marg[0], marg[1]


def test_nni_search():
    """The 8-taxon case of treenni_cases.search_case with the restatements as grad_fn and nni_fn.  Seed and S were chosen so that
    every start ends at the generating topology AND every decision is clear of 10 eps: the best delta of a round from the
    second best, and from eps itself (asserted here; the device run of test_gpu_treesearch.py must take the same moves)."""
    g, Q, prior, child, blen, c0 = NC.search_case()
    want = NC.clades(c0)
    assert [len(NC.clades(c) - want) for c in child] == [0, 1, 2, 3]
    out, gap, off = run_search(*NC.reference_fns(g, Q, prior), child, blen)
    print("moves", out['moves'], "rounds", out['rounds'], "margins %.3g %.3g" % (gap, off))
    assert gap > 1e-5 and off > 1e-5
    assert out['converged'].all()
    for t in range(4):
        assert NC.clades(out['child'][t]) == want, t
        assert (np.diff(out['history'][t]) >= 0).all() and len(out['history'][t]) == len(out['moves'][t]) + 1
        assert out['history'][t][-1] == out['loglik'][t] and out['rounds'][t] >= len(out['moves'][t])
    assert [len(m) for m in out['moves']][:2] == [0, 1]
    np.testing.assert_allclose(out['loglik'], out['loglik'][0], rtol=1e-9)   # one topology, one optimum


def test_search_reverts_a_move_that_does_not_pay():
    """toy functions: every tree is offered one move whose delta lies; the tree stays, the move is barred, the search ends"""
    child = np.array([[[0, 1], [3, 2]]], dtype=np.int32)
    calls = []

    def grad_fn(c, b):
        return np.full(len(c), -1.0 - 0.5 * (int(c[0, 0, 0]) != 0)), np.zeros(b.shape), np.full(b.shape, -1.0)

    def nni_fn(c, b):
        calls.append(1)
        d = np.full(b.shape, np.nan)
        d[:, 0, 0], d[:, 0, 1] = 0.5, -np.inf
        return np.full(len(c), -1.0), d

    out = nni_search(grad_fn, nni_fn, child, np.full((1, 2, 2), 0.1), max_rounds=5)
    assert out['converged'].all() and out['moves'] == [[]] and out['rounds'][0] == 1 and len(calls) == 2
    np.testing.assert_array_equal(out['child'], child)
    assert out['loglik'][0] == -1.0


# ---- (d) the runner's parser ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,what", [
    (['--score_search', 'nni'], '--score_search needs --score_trees and --score_opt true'),
    (['--score_search', 'nni', '--score_trees', 'x.nwk'], '--score_search needs --score_trees and --score_opt true'),
    (['--score_search', 'nni', '--score_trees', 'x.nwk', '--score_opt', 'true', '--score_rates', 'gamma:0.5:4'],
     '--score_search nni: the NNI neighbourhood is not built for rate mixtures'),
    (['--score_search', 'nni', '--score_trees', 'x.nwk', '--score_fit', 'branches+alpha', '--score_rates', 'gamma:0.5:4'],
     '--score_search nni: the NNI neighbourhood is not built for rate mixtures'),
    (['--score_search', 'spr', '--score_trees', 'x.nwk', '--score_opt', 'true'], "nni or nni:ROUNDS"),
    (['--score_search', 'nni:0', '--score_trees', 'x.nwk', '--score_opt', 'true'], "nni or nni:ROUNDS"),
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
    base = ['--dataset', 'primate_data_wang', '--score_trees', 'x.nwk', '--score_opt', 'true']
    assert runner.parse_args(base).score_search is None
    assert runner.parse_args(base + ['--score_search', 'nni']).score_search == ('nni', 20)
    assert runner.parse_args(base + ['--score_search', 'nni:3']).score_search == ('nni', 3)


# ---- the host half under sanitizers -------------------------------------------------------------------------------------------
def test_header_under_sanitizers(tmp_path):
    """The host half of phylo_treenni.h with a main of its own (tests/treenni_asan_main.cpp), address and undefined-behaviour
    sanitizers of the host compiler: host code, run as a program."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "treenni_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "phylo_amd", "csrc"), os.path.join(ROOT, "tests", "treenni_asan_main.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    assert b"0 values differ" in p.stdout
