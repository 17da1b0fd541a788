"""NNI neighbourhoods and NNI search under rate mixtures without a GPU: the NumPy restatement of
phylo_trees_nni_rates' contract (treenni_rates_ref.py) against the same formulas at 50 digits and against the restated mixture
log-likelihood of every explicitly built neighbour; its identities with the one-rate restatement; nni_search driven by restatements
under a rate model and its with_index form; the runner's parser; the host half of phylo_treenni_rates.h under sanitizers.

Every test here fails without phylo_trees_nni_rates in the binding, nni_search's with_index or the runner's --score_fit_search."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import treenni_cases as NC
import treenni_rates_cases as RC
import treenni_rates_ref as RR
import treenni_ref as NR
from phylo_amd import _ffi
from phylo_amd.treesearch import apply_nni, nni_moves, nni_search
from treegrad_cases import branch_matrices
from treegrad_rates_cases import MIX_I_G4, category_matrices

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_symbol_is_exported():
    assert 'phylo_trees_nni_rates' in _ffi.EXPORTS
    assert hasattr(_ffi.Context, 'trees_nni_rates')


# ---- (a) the restatement at 50 digits, and against explicit neighbours: E_NNI_RATES, E_EXPL_RATES ----------------------------------
def test_reference_against_mpmath():
    """Every move of the trees of treenni_cases.small_cases under three mixtures: p_inv 0.1 + Gamma4(0.5) (section 13b's; sites
    whose neighbour has f'_0 = 0 in the invariant class are among them, asserted), C = 1, and C = 16 (+I+G15).  E_NNI_RATES: the
    worst |restated delta - 50-digit delta| in units of (S + sum_s |d_s|) 2^-53.  E_EXPL_RATES: for loglik + delta against the
    restated mixture log-likelihood of apply_nni's tree, the errors of both sides against the 50-digit value of that tree, added,
    in units of (S + sum_s |log m_s| + sum_s |log m'_s|) 2^-53.  The 50-digit value of the move and of the explicit neighbour
    agree to 40 digits: the move IS that tree.  The figures measured here stand in treenni_rates_cases.py."""
    mp = pytest.importorskip("mpmath")
    worst_n, worst_x = {}, {}
    seen = zeros_seen = 0
    for mix_name, (rates, weights) in (('I+G4', MIX_I_G4), ('C1', RC.MIX_ONE), ('C16', RC.MIX_16)):
        wn = wx = 0.0
        for name, child, blen, Q, g in NC.small_cases():
            S = g.shape[1]
            M = category_matrices(Q, blen, rates)
            ll, delta, absd = RR.tree_nni_rates(child, M, NC.PRIOR, g, rates, weights)
            ell, eal, emv = RC.mp_tree_rates(mp, child, M, NC.PRIOR, g, weights)
            assert set(emv) == set(nni_moves(child)), name
            assert np.isnan(delta).sum() == delta.size - len(emv), name
            if rates[0] == 0:
                zeros_seen += sum(int((fp == 0).sum()) for fp in RR.category_factors(child, M[0], NC.PRIOR, g)[1].values())
            memo = {}
            for (r, sd), (ed, ea, dead) in emv.items():
                seen += 1
                if dead:                                                  # an impossible neighbour (zero-length branches)
                    assert delta[r, sd] == -np.inf, (mix_name, name, r, sd)
                    continue
                assert np.isfinite(delta[r, sd]), (mix_name, name, r, sd)
                err = float(abs(mp.mpf(float(delta[r, sd])) - ed) / ((S + ea) * mp.mpf(2) ** -53))
                assert abs(float(ea) - absd[r, sd]) <= 1e-9 * (1 + absd[r, sd])
                wn = max(wn, err)
                c2, b2 = apply_nni(child, blen, r, sd)
                M2 = np.array([NC.matrices_of(b2, blen, M[c]) for c in range(len(weights))])
                ll2, _ = RR.tree_loglik_sites(c2, M2, NC.PRIOR, g, weights)
                ell2, eal2 = RC.mp_loglik_rates(mp, c2, M2, NC.PRIOR, g, weights, memo)
                assert abs(ell2 - (ell + ed)) < mp.mpf(10) ** -40, (mix_name, name, r, sd)
                unit = (S + eal + eal2) * mp.mpf(2) ** -53
                both = float((abs(mp.mpf(float(ll + delta[r, sd])) - ell2) + abs(mp.mpf(ll2) - ell2)) / unit)
                wx = max(wx, both)
                assert abs((ll + delta[r, sd]) - ll2) <= RC.E_EXPL_RATES * float(unit), (mix_name, name, r, sd)
        worst_n[mix_name], worst_x[mix_name] = wn, wx
    print("restatement against 50 digits over %d moves: delta %s units (E_NNI_RATES = %g), explicit neighbours %s units "
          "(E_EXPL_RATES = %g); %d site factors of the invariant class are 0" % (seen, worst_n, RC.E_NNI_RATES, worst_x, RC.E_EXPL_RATES, zeros_seen))
    assert zeros_seen > 0
    assert RC.E_NNI_RATES / 2 <= max(worst_n.values()) <= RC.E_NNI_RATES
    assert RC.E_EXPL_RATES / 2 <= max(worst_x.values()) <= RC.E_EXPL_RATES


# ---- (b) identities with the one-rate restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", ["one", "half-half-16"])
def test_restatement_identities(mix):
    """C = 1 (rate 1, weight 1), and sixteen categories of which the two at positions 3 and 15 have rate 1 and weight 1/2 and the
    others weight 0: m = f and m' = f' exactly, so delta is treenni_ref.tree_nni's bit for bit"""
    rates, weights = RC.MIX_ONE if mix == "one" else RC.half_half_16()
    for name, child, blen, Q, g in NC.small_cases():
        ll0, d0, a0 = NR.tree_nni(child, branch_matrices(Q, blen), NC.PRIOR, g)
        ll, d, a = RR.tree_nni_rates(child, category_matrices(Q, blen, rates), NC.PRIOR, g, rates, weights)
        assert ll == ll0 and np.array_equal(d.view(np.uint64), d0.view(np.uint64)) and np.array_equal(a.view(np.uint64), a0.view(np.uint64)), name


# ---- (c) the search under a rate model ---------------------------------------------------------------------------------------------
def run_search(grad_fn, nni_fn, child, blen, eps=1e-6, **kw):
    """nni_search, with the margins of every decision: (result, least best - second-best delta of a taken move, least
    |best delta - eps|)"""
    marg = [np.inf, np.inf]

    def watched(c, b, *idx):
        ll, d = nni_fn(c, b, *idx)
        for x in np.asarray(d):
            f = np.sort(x[np.isfinite(x)])[::-1]
            marg[1] = min(marg[1], abs(f[0] - eps))
            if f[0] > eps:
                marg[0] = min(marg[0], f[0] - f[1])
        return ll, d

    return nni_search(grad_fn, watched, child, blen, max_rounds=10, eps=eps, **kw), marg[0], marg[1]


def test_nni_search_under_rates():
    """The 8-taxon case of treenni_rates_cases.search_case, simulated under Gamma4(0.5), with the restatements under that mixture
    as grad_fn and nni_fn.  Seed and S were chosen so that every start ends at the generating topology AND every decision is clear
    of 10 eps: the best delta of a round from the second best, and from eps itself (asserted here; the device run of
    test_gpu_treesearch_rates.py must take the same moves).  The climbs keep every length above treenni_rates_cases.SEARCH_LO (why:
    there).  Measured: margins 0.43 and 0.54."""
    g, Q, prior, child, blen, c0 = RC.search_case()
    want = NC.clades(c0)
    assert [len(NC.clades(c) - want) for c in child] == [0, 1, 2, 3]
    out, gap, off = run_search(*RC.reference_fns(g, Q, prior, *RC.SEARCH_MIX), child, blen, lo=RC.SEARCH_LO)
    print("moves", out['moves'], "rounds", out['rounds'], "margins %.3g %.3g" % (gap, off))
    assert gap > 1e-5 and off > 1e-5
    assert out['converged'].all()
    for t in range(4):
        assert NC.clades(out['child'][t]) == want, t
        assert (np.diff(out['history'][t]) >= 0).all() and len(out['history'][t]) == len(out['moves'][t]) + 1
        assert out['history'][t][-1] == out['loglik'][t] and out['rounds'][t] >= len(out['moves'][t])
    assert [len(m) for m in out['moves']][:2] == [0, 1]
    np.testing.assert_allclose(out['loglik'], out['loglik'][0], rtol=1e-9)   # one topology, one optimum


def test_with_index_on_shrinking_subsets():
    """with_index=True: grad_fn and nni_fn receive the indices, into the trees given, of the trees of that call.  Tree 1 finishes in
    round 1 (no move pays); trees 0 and 2 take a move in round 1 and finish in round 2: the subsets shrink and the indices follow."""
    child = np.array([[[0, 1], [2, 3], [4, 5]]] * 3, dtype=np.int32)
    blen = np.full((3, 3, 2), 0.1)
    pays = {0: 1, 1: 0, 2: 1}                               # moves that pay, per tree
    log = []
    state = {}

    def grad_fn(c, b, idx):
        assert idx.dtype == np.int64 and len(idx) == len(c) == len(b)
        log.append(('grad', idx.tolist()))
        ll = np.array([state.get((int(t), c[k].tobytes()), 0.0) for k, t in enumerate(idx)])
        return ll, np.zeros(b.shape), np.full(b.shape, -1.0)

    def nni_fn(c, b, idx):
        assert idx.dtype == np.int64 and len(idx) == len(c)
        log.append(('nni', idx.tolist()))
        d = np.full(b.shape, np.nan)
        d[:, :2, :] = -1.0
        for k, t in enumerate(idx):
            if pays[int(t)] > 0:
                d[k, 0, 0] = 0.5
                c2, _ = apply_nni(c[k], b[k], 0, 0)
                state[(int(t), c2.tobytes())] = state.get((int(t), c[k].tobytes()), 0.0) + 0.5
                pays[int(t)] -= 1
        return np.zeros(len(c)), d

    out = nni_search(grad_fn, nni_fn, child, blen, max_rounds=5, with_index=True)
    calls = [x for x in log if x[0] == 'nni']
    assert calls == [('nni', [0, 1, 2]), ('nni', [0, 2])]
    grads = [x[1] for x in log if x[0] == 'grad']
    assert grads[0] == [0, 1, 2] and [0, 2] in grads and all(gi in ([0, 1, 2], [0, 2]) for gi in grads)
    assert out['moves'] == [[(0, 0)], [], [(0, 0)]] and out['rounds'].tolist() == [1, 0, 1] and out['converged'].all()
    np.testing.assert_array_equal(out['loglik'], [0.5, 0.0, 0.5])


def test_default_call_is_unchanged():
    """without with_index the functions are called with two arguments, and the search of test_treenni_cpu's toy gives what it gave"""
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
    out2 = nni_search(lambda c, b, i: grad_fn(c, b), lambda c, b, i: nni_fn(c, b), child, np.full((1, 2, 2), 0.1), max_rounds=5, with_index=True)
    assert out2['moves'] == out['moves'] and out2['loglik'][0] == out['loglik'][0] == -1.0


# ---- (d) the runner's parser ---------------------------------------------------------------------------------------------------
FIT = ['--score_trees', 'x.nwk', '--score_rates', 'gamma:0.5:4', '--score_fit', 'branches+alpha']


@pytest.mark.parametrize("argv,what", [
    (['--score_fit_search', 'nni'], '--score_fit_search needs --score_trees, --score_rates and --score_fit'),
    (['--score_fit_search', 'nni', '--score_trees', 'x.nwk'], '--score_fit_search needs --score_trees, --score_rates and --score_fit'),
    (['--score_fit_search', 'nni', '--score_trees', 'x.nwk', '--score_rates', 'gamma:0.5:4'],
     '--score_fit_search needs --score_trees, --score_rates and --score_fit'),
    (['--score_fit_search', 'nni', '--score_rates', 'gamma:0.5:4', '--score_fit', 'branches+alpha'],
     '--score_fit_search needs --score_trees, --score_rates and --score_fit'),
    (['--score_fit_search', 'spr'] + FIT, "nni or nni:ROUNDS"),
    (['--score_fit_search', 'nni:0'] + FIT, "nni or nni:ROUNDS"),
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
    base = ['--dataset', 'primate_data_wang'] + FIT
    assert runner.parse_args(base).score_fit_search is None
    assert runner.parse_args(base + ['--score_fit_search', 'nni']).score_fit_search == ('nni', 20)
    assert runner.parse_args(base + ['--score_fit_search', 'nni:3']).score_fit_search == ('nni', 3)


# ---- the host half under sanitizers -------------------------------------------------------------------------------------------
def test_header_under_sanitizers(tmp_path):
    """The host half of phylo_treenni_rates.h (ptnr_make_plan, ptnr_lds_bytes) with a main of its own
    (tests/treenni_rates_asan_main.cpp), address and undefined-behaviour sanitizers of the host compiler: host code, run as a
    program."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "treenni_rates_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "phylo_amd", "csrc"), os.path.join(ROOT, "tests", "treenni_rates_asan_main.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    assert b"0 values differ" in p.stdout
