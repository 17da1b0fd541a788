"""Branch-length gradients without a GPU: the NumPy restatement of phylo_trees_grad's contract
(treegrad_ref.py) against central differences of the oracle's tree log-likelihood and against the same formulas at 50 digits;
phylo_amd.treeopt.optimize_branches driven by that restatement against scipy's L-BFGS-B; the runner's parser errors; the host
half of phylo_treegrad.h under sanitizers.

Every test here fails on import without phylo_amd.treeopt."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import treegrad_ref as TR
from oracle import cpu_ref as O
from phylo_amd import _ffi
from phylo_amd.treeopt import optimize_branches
from treegrad_cases import E_REF, branch_matrices, simulate
from trees_cases import random_rows, rows_to_nodes

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PRIOR = np.array([0.1, 0.2, 0.3, 0.4])


def gtr_Q(seed=7):
    return O.get_Q(np.random.default_rng(seed).normal(size=(4, 4)))


def gapped(N, S, rng):
    codes = rng.integers(0, 5, size=(N, S))
    return np.stack([(codes == b) | (codes == 4) for b in range(4)], axis=-1).astype(np.float64)


def test_symbol_is_exported():
    assert 'phylo_trees_grad' in _ffi.EXPORTS


# ---- (a) central differences of the oracle ----------------------------------------------------------------------------------
def test_reference_against_central_differences():
    """grad against (f(b + h) - f(b - h)) / 2h and curv against (f(b + h) - 2 f(b) + f(b - h)) / h^2 of oracle.cpu_ref.tree_loglik
    (scipy's expm on both sides), N = 6, S = 40, gaps, lengths 0.05 + Exp(0.1).  Measured here: h = 1e-5 gives the gradient to
    2e-9 of (1 + |value|) (truncation h^2 f''' / 6 and rounding eps |f| / h are both about 1e-9 there); h = 1e-3 gives the
    curvature to 2e-5 of (1 + |value|).  Asserted at 1e-7 and 1e-3: a wrong sign, a swapped side or row, or a missing term is off
    by its whole size."""
    N, S = 6, 40
    rng = np.random.default_rng(3)
    g = gapped(N, S, rng)
    Q = gtr_Q()
    child, blen = random_rows(N, rng, zeros=False)
    blen = blen + 0.05
    ll, grad, curv, _ = TR.tree_grad(child, branch_matrices(Q, blen), Q, PRIOR, g)

    def f(b):
        left, right, bl, br = rows_to_nodes(child, b)
        return O.tree_loglik(Q, PRIOR, 2 * N - 1, left, right, bl, br, 2 * N - 2, g)[0]

    assert ll == pytest.approx(f(blen), rel=1e-13)
    worst_g = worst_c = 0.0
    for i in range(N - 1):
        for sd in range(2):
            def at(h):
                b = blen.copy()
                b[i, sd] += h
                return f(b)
            fd = (at(1e-5) - at(-1e-5)) / 2e-5
            fd2 = (at(1e-3) - 2 * ll + at(-1e-3)) / 1e-6
            worst_g = max(worst_g, abs(fd - grad[i, sd]) / (1 + abs(fd)))
            worst_c = max(worst_c, abs(fd2 - curv[i, sd]) / (1 + abs(fd2)))
    print("central differences: gradient off by %.3g, curvature by %.3g of (1 + |value|)" % (worst_g, worst_c))
    assert worst_g <= 1e-7 and worst_c <= 1e-3


# ---- (b) the same formulas at 50 digits: E_REF --------------------------------------------------------------------------------
def test_reference_against_mpmath():
    """N = 5, S = 8, gaps; 20 random trees under a GTR-like Q and under JC69.  The worst |reference - 50-digit value| over every
    grad and curv entry, in units of (scale + |value|) 2^-53, is E_REF: the restatement's own error, from which the device
    tolerance 8 E_REF 2^-53 follows (treegrad_cases.py).  Measured here: 8.59 -- within-site cancellation in L' and the
    separately rounded M' = M Q are what it consists of."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    mpf = mp.mpf
    N, S = 5, 8
    worst = 0.0
    for seed in range(20):
        for jc in (False, True):
            rng = np.random.default_rng(seed)
            g = gapped(N, S, rng)
            Q = O.jc_Q() if jc else O.get_Q(rng.normal(size=(4, 4)))
            child, blen = random_rows(N, rng)
            M = branch_matrices(Q, blen)
            _, grad, curv, scale = TR.tree_grad(child, M, Q, PRIOR, g)
            Mm = [[[[mpf(float(v)) for v in r] for r in M[i, sd]] for sd in range(2)] for i in range(N - 1)]
            Qm = [[mpf(float(v)) for v in r] for r in Q]
            pm = [mpf(float(v)) for v in PRIOR]
            G = [[mpf(0), mpf(0)] for _ in range(N - 1)]
            Cv = [[mpf(0), mpf(0)] for _ in range(N - 1)]
            for s in range(S):
                rows = [[mpf(float(v)) for v in g[i, s]] for i in range(N)]
                L, d1, d2 = TR.site_terms(child.tolist(), Mm, Qm, pm, rows, mpf(0))
                for i in range(N - 1):
                    for sd in range(2):
                        G[i][sd] += d1[i][sd] / L
                        Cv[i][sd] += d2[i][sd] / L - (d1[i][sd] / L) ** 2
            for i in range(N - 1):
                for sd in range(2):
                    for val, exact in ((grad[i, sd], G[i][sd]), (curv[i, sd], Cv[i][sd])):
                        unit = (mpf(float(scale[i, sd])) + abs(exact)) * mpf(2) ** -53
                        worst = max(worst, float(abs(mpf(float(val)) - exact) / unit))
    print("reference against 50 digits: worst error %.3f units of (scale + |value|) 2^-53 (E_REF = %g)" % (worst, E_REF))
    assert E_REF / 2 <= worst <= E_REF


# ---- (c) the optimiser --------------------------------------------------------------------------------------------------------
def nni_neighbours(child):
    R = child.shape[0]
    N = R + 1
    parent = {int(child[p, sd]): (p, sd) for p in range(R) for sd in range(2)}
    out = []
    for i in range(R - 1):
        p, sd = parent[N + i]
        s = child[p, 1 - sd]
        if s < N + i:
            for k in range(2):
                c = child.copy()
                c[i, k], c[p, 1 - sd] = s, child[i, k]
                out.append(c)
    return out


@pytest.mark.parametrize("N,S,jc", [(5, 200, False), (5, 200, True), (8, 300, False), (8, 300, True)],
                         ids=['N5-gtr', 'N5-jc', 'N8-gtr', 'N8-jc'])
def test_optimize_branches_against_lbfgsb(N, S, jc):
    """An alignment simulated along a random tree; that tree and its nearest-neighbour interchanges, every length off by a
    factor in [1/2, 2].  The yardstick: scipy's L-BFGS-B on the same function from two different starts (the same perturbed
    lengths; 0.1 everywhere) agrees with itself to 2.6e-16 relative in the log-likelihood, measured here over the four cases
    -- one rounding of the value; it stops where the function's own rounding hides further progress.  The sum over up to 300
    sites rounds at about 2^-46 of its size (what treeopt.NOISE takes for it), so that is the bound both agreements are
    held to; optimize_branches was measured at 2.6e-16 against the yardstick."""
    from scipy.optimize import minimize
    Q = O.jc_Q() if jc else gtr_Q()
    prior = np.full(4, 0.25) if jc else PRIOR
    rng = np.random.default_rng(N)
    c0, b0 = random_rows(N, rng, zeros=False)
    g = simulate(c0, b0 + 0.05, Q, prior, S, rng)
    child = np.array([c0] + nni_neighbours(c0))
    T = child.shape[0]
    blen = b0[None] * rng.uniform(0.5, 2.0, size=(T, N - 1, 2))

    def fn(b):
        ll, grad, curv, _ = TR.trees_grad(child, branch_matrices(Q, b), Q, prior, g)
        return ll, grad, curv

    out = optimize_branches(fn, child, blen)
    print("iterations", out['iterations'])
    assert (np.diff(out['history'], axis=0) >= 0).all()                  # every tree's sequence is non-decreasing
    assert out['converged'].all() and (out['iterations'] <= 50).all()
    free = ~((out['blen'] <= 1e-8) & (out['grad'] < 0))
    assert (np.abs(out['grad'][free]) <= 1e-6).all()
    ll_end = fn(out['blen'])[0]
    np.testing.assert_allclose(ll_end, out['loglik'], rtol=2.0 ** -46, atol=0)
    worst_self = worst = 0.0
    for t in range(T):
        def f(x):
            ll, grad, _, _ = TR.tree_grad(child[t], branch_matrices(Q, x.reshape(N - 1, 2)), Q, prior, g)
            return -ll, -grad.ravel()
        runs = [minimize(f, start.ravel(), jac=True, method='L-BFGS-B', bounds=[(1e-8, 100.0)] * (2 * N - 2),
                         options=dict(gtol=1e-6, ftol=0, maxiter=1000)) for start in (blen[t], np.full((N - 1, 2), 0.1))]
        worst_self = max(worst_self, abs(runs[0].fun - runs[1].fun) / abs(runs[0].fun))
        best = -min(r.fun for r in runs)
        worst = max(worst, abs(out['loglik'][t] - best) / abs(best))
    print("L-BFGS-B against itself: %.3g relative; optimize_branches against it: %.3g" % (worst_self, worst))
    assert worst_self <= 2.0 ** -46 and worst <= 2.0 ** -46


def test_optimizer_keeps_lengths_of_converged_trees_and_bounds():
    """a concave toy function with its optimum outside [lo, hi] on one branch: that branch ends at the bound, the tree converges"""
    target = np.array([[[0.3, 200.0], [1e-12, 0.7]]])

    def fn(b):
        return -((b - target) ** 2).sum(axis=(1, 2)), -2 * (b - target), np.full(b.shape, -2.0)

    out = optimize_branches(fn, None, np.full((1, 2, 2), 0.5))
    assert out['converged'].all()
    np.testing.assert_allclose(out['blen'], [[[0.3, 100.0], [1e-8, 0.7]]], rtol=1e-9)
    assert (np.diff(out['history'], axis=0) >= 0).all()


# ---- (d) the runner's parser ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,what", [
    (['--score_opt', 'true'], '--score_opt true needs --score_trees'),
    (['--score_opt', 'true', '--score_trees', 'x.nwk', '--score_rates', 'gamma:0.5:4'], 'not built for rate mixtures'),
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
    ok = runner.parse_args(['--dataset', 'primate_data_wang', '--score_trees', 'x.nwk', '--score_opt', 'true'])
    assert ok.score_opt is True and runner.parse_args(['--dataset', 'primate_data_wang']).score_opt is False


# ---- the host half under sanitizers -------------------------------------------------------------------------------------------
def test_header_under_sanitizers(tmp_path):
    """The host half of phylo_treegrad.h with a main of its own (tests/treegrad_asan_main.cpp), address and undefined-behaviour
    sanitizers of the host compiler: host code, run as a program."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "treegrad_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "phylo_amd", "csrc"), os.path.join(ROOT, "tests", "treegrad_asan_main.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    assert b"0 values differ" in p.stdout
