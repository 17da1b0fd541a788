"""Model gradients without a GPU: the NumPy restatement of phylo_trees_grad_model's contract
(treegrad_model_ref.py) against the same formulas at 50 digits, which sets the device tolerance; phylo_amd.modelfit against
central differences at 50 digits; phylo_amd.treeopt.optimize_model driven by the restatement against scipy's L-BFGS-B; the
runner's parser errors; the host half of phylo_treegrad_model.h under sanitizers.

Every test here fails on import without phylo_amd.modelfit."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import treegrad_model_cases as MC
import treegrad_model_ref as MR
import treegrad_ref as TR
from oracle import cpu_ref as O
from phylo_amd import _ffi, model, modelfit
from phylo_amd.treeopt import optimize_model
from treegrad_cases import branch_matrices
from trees_cases import random_rows

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PRIOR = np.array([0.1, 0.2, 0.3, 0.4])


def gapped(N, S, rng):
    codes = rng.integers(0, 5, size=(N, S))
    return np.stack([(codes == b) | (codes == 4) for b in range(4)], axis=-1).astype(np.float64)


def test_symbol_is_exported():
    assert 'phylo_trees_grad_model' in _ffi.EXPORTS


# ---- 1. the same formulas at 50 digits: E_REF_MODEL ---------------------------------------------------------------------------
def test_reference_against_mpmath():
    """Section 13's recipe: N = 5, S = 8, gaps; 20 random trees under a GTR-like Q and under JC69 (the generator of the closed
    form).  Directions: the 12 softmax directions of a random y_q, Q itself, one random direction.  The yardstick takes the SAME
    inputs (M, the doubles Q, dirs, t) and makes D from mpmath.expm of the 8 x 8 block matrix [[A, E], [0, A]], A = Q t and
    E = dirs[p] t, every sum at 50 digits.  The worst |reference - 50-digit value| over every dtheta and dprior entry, in units
    of (scale + |value|) 2^-53 -- scale = sum_s sum_b |l_{p,b}[s]| for dtheta, sum_s x_root[j] / L_s for dprior --, is
    E_REF_MODEL, from which TOL_MODEL = 8 E_REF_MODEL 2^-53 follows (treegrad_model_ref.py)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    mpf = mp.mpf
    N, S = 5, 8
    worst_t = worst_p = 0.0

    cache = {}

    def exact_D(Qe, E, t):
        if t == 0.0:
            return [[mpf(0)] * 4 for _ in range(4)]
        key = (Qe.tobytes(), E.tobytes(), float(t))                      # one expm per distinct (generator, direction, length)
        if key not in cache:
            cache[key] = exact_D_of(Qe, E, t)
        return cache[key]

    def exact_D_of(Qe, E, t):
        B = mp.zeros(8, 8)
        for i in range(4):
            for j in range(4):
                a = mpf(float(Qe[i, j])) * mpf(float(t))
                B[i, j] = a
                B[4 + i, 4 + j] = a
                B[i, 4 + j] = mpf(float(E[i, j])) * mpf(float(t))
        X = mp.expm(B)
        return [[X[i, 4 + j] for j in range(4)] for i in range(4)]

    for seed in range(20):
        for jc in (False, True):
            rng = np.random.default_rng(seed)
            g = gapped(N, S, rng)
            Q = O.jc_Q() if jc else O.get_Q(rng.normal(size=(4, 4)))
            child, blen = random_rows(N, rng)
            y = rng.normal(size=(4, 4))
            dirs = np.concatenate([modelfit.q_directions(y), Q[None], rng.normal(size=(1, 4, 4))])
            P = dirs.shape[0]
            M = branch_matrices(Q, blen)
            D = MR.direction_matrices(Q, dirs, blen, jc=jc)
            assert (D[blen == 0] == 0).all()                                  # a zero-length branch: D = 0 exactly
            _, dth, dpr, sc_t, sc_p = MR.tree_grad_model(child, M, D, PRIOR, g)
            Mm = [[[[mpf(float(v)) for v in r] for r in M[i, sd]] for sd in range(2)] for i in range(N - 1)]
            Dm = [[[exact_D(Q, dirs[p], blen[i, sd]) for p in range(P)] for sd in range(2)] for i in range(N - 1)]
            pm = [mpf(float(v)) for v in PRIOR]
            Th, Ta = [mpf(0)] * P, [mpf(0)] * P
            Pr = [mpf(0)] * 4
            for s in range(S):
                rows = [[mpf(float(v)) for v in g[i, s]] for i in range(N)]
                L, tot, tot_abs, xr = MR.site_terms_model(child.tolist(), Mm, Dm, pm, rows, mpf(0))
                for p in range(P):
                    Th[p] += tot[p] / L
                for j in range(4):
                    Pr[j] += xr[j] / L
            for p in range(P):
                unit = (mpf(float(sc_t[p])) + abs(Th[p])) * mpf(2) ** -53
                worst_t = max(worst_t, float(abs(mpf(float(dth[p])) - Th[p]) / unit))
            for j in range(4):
                unit = (mpf(float(sc_p[j])) + abs(Pr[j])) * mpf(2) ** -53
                worst_p = max(worst_p, float(abs(mpf(float(dpr[j])) - Pr[j]) / unit))
    worst = max(worst_t, worst_p)
    print("reference against 50 digits: worst error %.3f units of (scale + |value|) 2^-53 (dtheta %.3f, dprior %.3f; E_REF_MODEL = %g)"
          % (worst, worst_t, worst_p, MR.E_REF_MODEL))
    assert MR.E_REF_MODEL / 2 <= worst <= MR.E_REF_MODEL
    assert MR.TOL_MODEL == 8 * MR.E_REF_MODEL * 2.0 ** -53


def test_frechet_restatement_against_scipy():
    """the restated series against scipy's expm_frechet over norms that take every term count and several squarings"""
    from scipy.linalg import expm_frechet
    rng = np.random.default_rng(5)
    A = np.array([O.get_Q(rng.normal(size=(4, 4))) * t for t in (0.0, 0.004, 0.02, 0.06, 0.12, 0.2, 0.4, 1.5, 7.0, 40.0)])
    E = rng.normal(size=A.shape)
    L = MR.frechet(A, E)
    for a, e, l in zip(A, E, L):
        ref = expm_frechet(a, e, compute_expm=False)
        assert np.abs(l - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
    assert (MR.frechet(A[:1], E[:1] * 0.0) == 0).all()


# ---- 2. modelfit against central differences at 50 digits ---------------------------------------------------------------------
def test_q_directions_and_chain_prior_against_differences():
    """get_Q and get_stationary_probs restated in mpmath, central differences with h = 1e-20 at 50 digits (truncation ~1e-40):
    q_directions and chain_prior are exact formulas, held to a few roundings (1e-15 of the largest entry)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    mpf = mp.mpf
    rng = np.random.default_rng(11)
    y = rng.normal(size=(4, 4))
    ys = rng.normal(size=4)

    def get_Q_mp(ym):
        Q = [[mpf(0)] * 4 for _ in range(4)]
        for a in range(4):
            z = sum(mp.exp(ym[a][c]) for c in range(4) if c != a)
            for c in range(4):
                if c != a:
                    Q[a][c] = mp.exp(ym[a][c]) / z
            Q[a][a] = -sum(Q[a][c] for c in range(4) if c != a)
        return Q

    np.testing.assert_allclose(np.array([[float(v) for v in r] for r in get_Q_mp([[mpf(float(v)) for v in r] for r in y])]),
                               model.get_Q(y), rtol=1e-14, atol=1e-16)
    h = mpf(10) ** -20
    dirs = modelfit.q_directions(y)
    assert dirs.shape == (12, 4, 4) and len(modelfit.OFFDIAG) == 12
    for p, (a, b) in enumerate(modelfit.OFFDIAG):
        up = [[mpf(float(v)) for v in r] for r in y]
        dn = [[mpf(float(v)) for v in r] for r in y]
        up[a][b] += h
        dn[a][b] -= h
        Qu, Qd = get_Q_mp(up), get_Q_mp(dn)
        fd = np.array([[float((Qu[i][j] - Qd[i][j]) / (2 * h)) for j in range(4)] for i in range(4)])
        assert np.abs(dirs[p] - fd).max() <= 1e-15, (a, b)
    np.testing.assert_array_equal(modelfit.unpack_q(modelfit.pack_q(y)), y - np.diag(np.diag(y)))
    # chain_prior: d/dy_k of sum_j w_j softmax(y)_j for weights w = dprior
    w = rng.normal(size=4)

    def f(yv):
        e = [mp.exp(v) for v in yv]
        z = sum(e)
        return sum(mpf(float(w[j])) * e[j] / z for j in range(4))

    got = modelfit.chain_prior(w, ys)
    for k in range(4):
        up = [mpf(float(v)) for v in ys]
        dn = [mpf(float(v)) for v in ys]
        up[k] += h
        dn[k] -= h
        assert abs(got[k] - float((f(up) - f(dn)) / (2 * h))) <= 1e-15
    assert abs(got.sum()) <= 1e-15                                            # no component along (1, 1, 1, 1)
    np.testing.assert_allclose(modelfit.chain_prior(np.stack([w, 2 * w]), ys), np.stack([got, 2 * got]), rtol=1e-14, atol=1e-16)


def test_restated_gradient_against_differences_of_the_loglik():
    """dtheta along the softmax directions and chain_prior(dprior) against central differences of the restated log-likelihood in
    y_q and y_station (h = 1e-5: truncation and rounding both near 1e-9 of (1 + |value|); asserted at 1e-7)"""
    N, S = 6, 40
    rng = np.random.default_rng(3)
    g = gapped(N, S, rng)
    y, ys = rng.normal(size=(4, 4)), rng.normal(size=4)
    np.fill_diagonal(y, 0.0)
    child, blen = random_rows(N, rng, zeros=False)
    blen = blen + 0.05

    def f(yq, yst):
        Q = model.get_Q(yq)
        return TR.tree_grad(child, branch_matrices(Q, blen), Q, model.get_stationary_probs(yst).reshape(4), g)[0]

    Q, pi = model.get_Q(y), model.get_stationary_probs(ys).reshape(4)
    dirs = modelfit.q_directions(y)
    ll, dth, dpr, _, _ = MR.tree_grad_model(child, branch_matrices(Q, blen), MR.direction_matrices(Q, dirs, blen), pi, g)
    assert ll == f(y, ys)
    h = 1e-5
    for p, (a, b) in enumerate(modelfit.OFFDIAG):
        e = np.zeros((4, 4))
        e[a, b] = h
        fd = (f(y + e, ys) - f(y - e, ys)) / (2 * h)
        assert abs(fd - dth[p]) <= 1e-7 * (1 + abs(fd)), (a, b, fd, dth[p])
    gs = modelfit.chain_prior(dpr, ys)
    for k in range(4):
        e = np.zeros(4)
        e[k] = h
        fd = (f(y, ys + e) - f(y, ys - e)) / (2 * h)
        assert abs(fd - gs[k]) <= 1e-7 * (1 + abs(fd)), (k, fd, gs[k])


# ---- 3. the optimiser ---------------------------------------------------------------------------------------------------------
def test_optimize_model_against_lbfgsb():
    """The simulated case of treegrad_model_cases.fit_case(): 8 taxa, 600 sites, the tree and four NNI neighbours; the model
    starts at the uniform row-softmax Q and the uniform pi.  The functions are the restatements under the TEXTBOOK pruning
    convention (treegrad_model_cases.host_fns(textbook=True): the same code with every matrix transposed), the convention the
    alignment was simulated under and the one under which a row-softmax Q gives probabilities: the objective then has an
    interior maximum, and agreement between climbers means something.  (Under the project's own convention it has none:
    test_optimize_model_under_the_projects_convention)

    The objective never falls, and is the sum of the returned log-likelihoods; it ends at or above the objective of the TRUE
    model and lengths; the gradient of the model coordinates AT the returned model and lengths is below 10 gtol (gtol = 1e-6 is
    the rule the BFGS stops by; the last climb of the lengths moves the point once more, by less than a round's rise of tol =
    1e-11 allows).  The yardstick: scipy's L-BFGS-B (30 pairs, gtol 1e-9, ftol 0) on the joint function of the model
    coordinates and the lengths of the fit_on tree, from two starts.  Its own relative spread between the starts and
    optimize_model's distance from the better of them, on EITHER side, are both held to FIT_MARGIN = 2^-46.

    Measured: 8 rounds, -4413.765848 -> -4269.907955722420, |g| 9.4e-7 at the end; the true model and lengths score -4279.95;
    L-BFGS-B ends at -4269.907955722421 and ...423 (4.7e-16 apart, relative); optimize_model lies 2.1e-16 from the better."""
    from scipy.optimize import minimize
    case = MC.fit_case()
    child, blen, g, N, S = case['child'], case['blen'], case['g'], case['N'], case['S']
    grad_fn, grad_model_fn = MC.host_fns(child, g, textbook=True)
    gtol = 1e-6
    out = optimize_model(grad_model_fn, grad_fn, child, blen, case['y_q0'], case['y_station0'], fit=('q', 'pi'), tol=1e-11, max_rounds=60,
                         gtol=gtol)
    print("rounds %d, fit_on %r, objective %.12f -> %.12f, |g| %.3g" % (out['rounds'], out['fit_on'], out['objective_start'],
                                                                        out['objective'], np.abs(out['grad_model']).max()))
    assert out['converged'] and out['fit_on'] == [0]                          # the tree the alignment was simulated on scores best
    assert (np.diff(out['history']) >= 0).all()                               # (nothing in optimize_model forces this: a half round that
    assert out['history'][0] == out['objective_start'] and out['history'][-1] == out['objective']      # lowers it is refused, not hidden)
    assert out['objective'] == out['loglik'][out['fit_on']].sum()
    t = out['fit_on'][0]
    Qt = case['Q'].T
    truth = TR.tree_grad(child[t], branch_matrices(Qt, case['true_blen']), Qt, case['pi'], g)[0]
    print("objective at the true model and lengths %.6f" % truth)
    assert out['objective'] >= truth
    assert np.abs(out['grad_model']).max() <= 10 * gtol
    ll_end = grad_fn(out['blen'], out['Q'], out['pi'])[0]
    np.testing.assert_allclose(ll_end, out['loglik'], rtol=2.0 ** -46, atol=0)    # (optimize_branches keeps the larger of two values inside NOISE)
    np.testing.assert_allclose(out['Q'].sum(axis=1), 0, atol=1e-15)
    np.testing.assert_allclose(out['Q'], model.get_Q(out['y_q']), rtol=0, atol=0)
    np.testing.assert_allclose(out['Q'], case['Q'], atol=0.06)                # ... and it is the model the data came from, within
    np.testing.assert_allclose(out['pi'], case['pi'], atol=0.03)              # what 600 sites tell (measured: 0.046 and 0.015)

    nb = 2 * (N - 1)

    grad_fn1, grad_model_fn1 = MC.host_fns(child[t:t + 1], g, textbook=True)

    def f(x):                                                                 # the joint function of the fit_on tree alone
        yq, ys, b = modelfit.unpack_q(x[:12]), x[12:16], x[16:].reshape(1, N - 1, 2)
        Q, pi = model.get_Q(yq), model.get_stationary_probs(ys).reshape(4)
        ll, grad, _ = grad_fn1(b, Q, pi)
        _, dth, dpr = grad_model_fn1(np.array([0]), b, Q, pi, modelfit.q_directions(yq))
        return -ll[0], -np.concatenate([dth[0], modelfit.chain_prior(dpr[0], ys), grad[0].ravel()])

    bounds = [(None, None)] * 16 + [(1e-8, 100.0)] * nb
    starts = (np.concatenate([modelfit.pack_q(case['y_q0']), case['y_station0'], blen[t].ravel()]),
              np.concatenate([modelfit.pack_q(case['y_q']), case['y_station'], np.full(nb, 0.1)]))
    runs = [minimize(f, s, jac=True, method='L-BFGS-B', bounds=bounds, options=dict(gtol=1e-9, ftol=0, maxiter=5000, maxcor=30, maxls=50))
            for s in starts]
    spread = abs(runs[0].fun - runs[1].fun) / abs(runs[0].fun)
    best = -min(r.fun for r in runs)
    dist = abs(best - out['objective']) / abs(best)
    print("L-BFGS-B %.12f and %.12f: %.3g apart, relative; optimize_model %.3g from the better run (FIT_MARGIN %.3g)"
          % (-runs[0].fun, -runs[1].fun, spread, dist, MC.FIT_MARGIN))
    assert spread <= MC.FIT_MARGIN and dist <= MC.FIT_MARGIN


def test_optimize_model_under_the_projects_convention():
    """The same case and start under the project's OWN pruning convention (a message is x . M): the host run of
    the fit the device test makes (test_gpu_modelfit.py compares with FIT_OBJECTIVE_HOST and runs no host fit).  The best tree
    alone is passed: trees climb independently of one another and the objective is that tree's, so its path is the five trees'.
    Here the site factors of an asymmetric Q are not probabilities and the objective has no interior maximum: the fit climbs from
    -4413.77 to -3183.42 in 16 rounds, 1159 above the model the data were simulated under (-4342.48), and ends on the boundary
    of the softmax, pi = (0, 1, 0, 0).  Nothing is compared with another climber on this function."""
    case = MC.fit_case()
    child, blen, g = case['child'][:1], case['blen'][:1], case['g']
    grad_fn, grad_model_fn = MC.host_fns(child, g)
    out = optimize_model(grad_model_fn, grad_fn, child, blen, case['y_q0'], case['y_station0'], fit=('q', 'pi'))
    print("rounds %d, objective %.12f -> %.12f (FIT_OBJECTIVE_HOST %.12f)" % (out['rounds'], out['objective_start'], out['objective'],
                                                                             MC.FIT_OBJECTIVE_HOST))
    assert out['converged'] and (np.diff(out['history']) >= 0).all()
    assert out['objective'] == out['loglik'][out['fit_on']].sum()
    assert abs(out['objective'] - MC.FIT_OBJECTIVE_HOST) <= MC.FIT_MARGIN * abs(MC.FIT_OBJECTIVE_HOST)
    truth = TR.tree_grad(child[0], branch_matrices(case['Q'], case['true_blen']), case['Q'], case['pi'], g)[0]
    assert out['objective'] > truth + 1000                                    # no likelihood of 600 sites lies this far above the truth's
    np.testing.assert_allclose(out['pi'], [0, 1, 0, 0], atol=1e-6)


def test_optimize_model_refuses_a_bad_fit():
    with pytest.raises(ValueError):
        optimize_model(None, None, None, np.zeros((1, 2, 2)), model.init_y_q(), np.zeros(4), fit=('pi',))
    with pytest.raises(ValueError):
        optimize_model(None, None, None, np.zeros((1, 2, 2)), model.init_y_q(), np.zeros(4), fit=('q', 'alpha'))


# ---- 4. the host half under sanitizers ----------------------------------------------------------------------------------------
def test_header_under_sanitizers(tmp_path):
    """The host half of phylo_treegrad_model.h with a main of its own (tests/treegrad_model_asan_main.cpp), address and
    undefined-behaviour sanitizers of the host compiler: host code, run as a program."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "treegrad_model_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "phylo_amd", "csrc"), os.path.join(ROOT, "tests", "treegrad_model_asan_main.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    assert b"0 checks failed" in p.stdout


# ---- 5. the runner's parser, and the run without the flag ---------------------------------------------------------------------
def _runner():
    sys.path.insert(0, ROOT)
    try:
        import runner
    finally:
        sys.path.remove(ROOT)
    return runner


@pytest.mark.parametrize("argv,what", [
    (['--score_model_fit', 'q'], '--score_model_fit needs --score_trees and --score_opt true'),
    (['--score_model_fit', 'q', '--score_trees', 'x.nwk'], '--score_model_fit needs --score_trees and --score_opt true'),
    (['--score_model_fit', 'q+pi', '--score_trees', 'x.nwk', '--score_rates', 'gamma:0.5:4'], 'not built for rate mixtures'),
    (['--score_model_fit', 'q', '--score_trees', 'x.nwk', '--score_rates', 'gamma:0.5:4', '--score_fit', 'branches'],
     'not built for rate mixtures'),
    (['--score_model_fit', 'q', '--score_trees', 'x.nwk', '--score_opt', 'true', '--score_search', 'nni'],
     'the NNI search runs under the model given'),
    (['--score_model_fit', 'pi', '--score_trees', 'x.nwk', '--score_opt', 'true'], 'invalid choice'),
])
def test_runner_parser_errors(argv, what, capsys):
    runner = _runner()
    with pytest.raises(SystemExit) as e:
        runner.parse_args(['--dataset', 'primate_data_wang'] + argv)
    assert e.value.code == 2 and what in capsys.readouterr().err


def test_runner_without_the_flag_is_what_it_was(tmp_path):
    """the parser's result and run_parameters.txt (the one score-tree output a run reaches without a device) carry nothing of the
    flag when it is absent"""
    runner = _runner()
    from phylo_amd.datasets import load_dataset
    from phylo_amd.vcsmc import VCSMC
    base = ['--dataset', 'primate_data_wang', '--score_trees', 'x.nwk', '--score_opt', 'true']
    off, on = runner.parse_args(base), runner.parse_args(base + ['--score_model_fit', 'q+pi'])
    assert off.score_model_fit is None and on.score_model_fit == 'q+pi'
    assert {k: v for k, v in vars(on).items() if k != 'score_model_fit'} == {k: v for k, v in vars(off).items() if k != 'score_model_fit'}
    text = {}
    for name, args in (('off', off), ('on', on)):
        v = VCSMC(load_dataset('primate_data_wang'), K=4, args=args)
        v.lr = 0.001
        d = tmp_path / name
        v._save_results(str(d), 0.0, {k: [] for k in ('cost', 'log_weights', 'Qmatrices', 'left_branches', 'right_branches', 'log_lik',
                                                      'll_tilde', 'log_lik_R', 'jump_chain_evolution', 'newick')})
        text[name] = (d / 'run_parameters.txt').read_text()
    assert 'score_model_fit' not in text['off'] and 'score_model_fit : q+pi' in text['on']
    assert text['on'].replace('score_model_fit : q+pi\n', '') == text['off']
    with pytest.raises(ValueError):
        VCSMC(load_dataset('primate_data_wang'), K=4, args=off).score_trees(['x'], fit_model=('q',))
