"""phylo_trees_grad on the device: the derivatives of the log-likelihood of a set of trees with respect
to every branch length.  loglik is held to phylo_trees_loglik's bits; grad and curv to the NumPy restatement (treegrad_ref.py,
fed with the device's own branch matrices) within TOL (scale + |value|), TOL = 8 E_REF 2^-53 with E_REF the restatement's own
error against 50-digit arithmetic (treegrad_cases.py) -- a bound set before the kernel ran.  Then: repeated and chunked calls
bit for bit, what the call leaves alone, refusals, the NaN rule, the optimiser on the device, runner.py --score_opt.

Every test here needs Context.trees_grad: AttributeError without it."""
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import treegrad_ref as TR
from oracle import cpu_ref as O
from phylo_amd import _ffi, model
from phylo_amd import treepost as TP
from phylo_amd.datasets import load_dataset
from phylo_amd.treeopt import optimize_branches
from test_gpu_trees_loglik import CASES, PI, alignment, bits, gtr_Q, make_ctx, random_trees, shaped_trees
from treegrad_cases import TOL, simulate
from trees_cases import random_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
T = 37
PRIOR = np.array([0.1, 0.2, 0.3, 0.4])


def reference(ctx, child, blen, Q, prior, g):
    """the restatement on the device's own matrices (ctx.expm_batched): expm differences stay out of the comparison"""
    M = ctx.expm_batched(blen.reshape(-1)).reshape(blen.shape + (4, 4))
    return TR.trees_grad(child, M, Q, prior, g)


def close(name, got, ref, scale):
    err = np.abs(got - ref) / (scale + np.abs(ref))
    print("%s: worst |device - reference| / (scale + |value|) = %.3g (TOL %.3g)" % (name, np.nanmax(err), TOL))
    assert np.isfinite(got).all(), name
    assert (err <= TOL).all(), (name, float(np.nanmax(err)), TOL)


# ---- 1. the cases of section 11, several chunks each ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_reference(name, monkeypatch):
    kw = CASES[name]
    N, S, jc, n = kw['N'], kw['S'], kw.get('jc', False), kw.get('n', T)
    g = alignment(N, S, 100 + N + S, kw.get('gaps', False), kw.get('generic', False))
    Q = O.jc_Q() if jc else gtr_Q()
    child, blen = shaped_trees(kw['shape'], N, 5, n) if 'shape' in kw else random_trees(N, 5, n)
    if N > 2:
        assert (blen == 0).any()                                          # trees with zero-length branches
    monkeypatch.setenv('PHYLO_TREES_CHUNK', '2' if n < T else '5')        # read when the context is created: several chunks
    with make_ctx(g, Q, jc=jc, tile=kw.get('tile')) as ctx:
        ll, grad, curv = ctx.trees_grad(child, blen, prior=PRIOR, want_curv=True)
        st = ctx.last_trees_stats
        assert st['units'] == n * S * (N - 1) and st['sweep_ms'] > 0
        per_chunk = 5 if kw.get('generic') else 6                         # coded leaves: the gap rows of M too
        assert st['n_launches'] == -(-n // (2 if n < T else 5)) * per_chunk
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)), err_msg="loglik against phylo_trees_loglik")
        assert np.isfinite(ll).all()
        ll2, grad_only = ctx.trees_grad(child, blen, prior=PRIOR)          # without curvature: the same gradient bits
        np.testing.assert_array_equal(bits(ll2), bits(ll))
        np.testing.assert_array_equal(bits(grad_only), bits(grad))
        rll, rgrad, rcurv, scale = reference(ctx, child, blen, Q, PRIOR, g)
        np.testing.assert_allclose(ll, rll, rtol=1e-12, atol=0)
        close(name + " grad", grad, rgrad, scale)
        close(name + " curv", curv, rcurv, scale)
        rev = ctx.trees_grad(child[::-1], blen[::-1], prior=PRIOR, want_curv=True)   # a tree's bits do not depend on its place
        for a, b in zip(rev, (ll, grad, curv)):
            np.testing.assert_array_equal(bits(a[::-1]), bits(b))


def test_prior_none_is_the_models_pi():
    g = alignment(7, 70, 3, gaps=True)
    pi = np.array([0.4, 0.3, 0.2, 0.1])
    child, blen = random_trees(7, 9, 5)
    with make_ctx(g, gtr_Q(), pi=pi) as ctx:
        a, b = ctx.trees_grad(child, blen, want_curv=True), ctx.trees_grad(child, blen, prior=pi, want_curv=True)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(bits(x), bits(y))
        assert not np.array_equal(a[1], ctx.trees_grad(child, blen, prior=PI)[1])


# ---- 2. the same bits again, and in chunks ----------------------------------------------------------------------------------
def test_two_calls_and_chunks_give_the_same_bits(monkeypatch):
    g = alignment(12, 130, 31, gaps=True)
    child, blen = random_trees(12, 6)
    got = {}
    for chunk in ('0', '5', '1'):
        monkeypatch.setenv('PHYLO_TREES_CHUNK', chunk)
        with make_ctx(g, gtr_Q(), tile=64) as ctx:
            got[chunk] = ctx.trees_grad(child, blen, want_curv=True)
            launches = ctx.last_trees_stats['n_launches']
            again = ctx.trees_grad(child, blen, want_curv=True)
            for a, b in zip(again, got[chunk]):
                np.testing.assert_array_equal(bits(a), bits(b))
        assert launches == 6 * {'0': 1, '5': 8, '1': 37}[chunk]
    for chunk in ('5', '1'):
        for a, b in zip(got[chunk], got['0']):
            np.testing.assert_array_equal(bits(a), bits(b))


# ---- 3. what the call leaves alone ------------------------------------------------------------------------------------------
def test_sweep_backward_summary_and_scratch_are_left_alone():
    g = load_dataset('primate_data')['genome'][:6, 100:170].copy()
    N, S, K, seed = 6, 70, 64, 5
    pi = np.array([[0.3, 0.2, 0.2, 0.3]])
    Q = model.get_Q(model.init_y_q())
    lam = np.linspace(5.0, 15.0, N - 1)
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, pi, lam, lam[::-1].copy())
        out = ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        grad = ctx.sweep_backward()
        ctx.sweep_async(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        child, blen = TP.particle_trees(out['merges'], out['ancestors'], out['left_branches'], out['right_branches'], seed=seed)
        ll, sites = ctx.trees_loglik(child[:7], blen[:7], want_sites=True)
        rl = ctx.rell(sites, 50, 3, want_reps=True)
        tll, tgrad, tcurv = ctx.trees_grad(child, blen, want_curv=True)     # between a sweep and its pending reverse pass
        assert np.isfinite(tgrad).all() and np.isfinite(tcurv).all()
        np.testing.assert_array_equal(bits(tll[:7]), bits(ll))
        grad2 = ctx.sweep_backward()
        again = ctx.sweep_fetch()
        for key in ('log_weights', 'log_likelihood', 'left_branches', 'right_branches'):
            np.testing.assert_array_equal(bits(again[key]), bits(out[key]), err_msg=key)
        np.testing.assert_array_equal(again['ancestors'], out['ancestors'])
        assert bits(again['logZ']) == bits(out['logZ'])
        for key in ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q'):
            np.testing.assert_array_equal(bits(grad2[key]), bits(grad[key]), err_msg=key)
        # the scratch of sections 11 and 12: the same calls give the same bits afterwards
        l2, s2 = ctx.trees_loglik(child[:7], blen[:7], want_sites=True)
        np.testing.assert_array_equal(bits(s2), bits(sites))
        np.testing.assert_array_equal(bits(ctx.rell(sites, 50, 3, want_reps=True)['rep_loglik']), bits(rl['rep_loglik']))
        # a tree summary made before the call still has its branch pass
        tab = ctx.tree_summary()
        ctx.trees_grad(child[:3], blen[:3])
        tb = ctx.tree_branches(tab)
        assert np.isfinite(tb['leaf_stats']).all()
        third = ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)   # the next sweep's bits
        np.testing.assert_array_equal(bits(third['log_weights']), bits(out['log_weights']))


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing():
    N, S = 5, 70
    g = alignment(N, S, 41)
    child, blen = random_trees(N, 8, 4)
    child[2] = np.array([[0, 1], [2, 3], [6, 4], [5, 7]], dtype=np.int32)
    with _ffi.Context(4, N, S) as ctx:
        with pytest.raises(_ffi.PhyloError) as e:
            ctx.trees_grad(child, blen)
        assert e.value.code == -6
        ctx.set_leaves(g)
        ctx.set_model(gtr_Q(), PI, np.full(N - 1, 10.0), np.full(N - 1, 10.0))
        ref = ctx.trees_grad(child, blen, want_curv=True)

        def refused(call, what):
            with pytest.raises(_ffi.PhyloError) as e:
                call()
            assert e.value.code == -1 and what in str(e.value), str(e.value)
            for a, b in zip(ctx.trees_grad(child, blen, want_curv=True), ref):            # a valid call still works
                np.testing.assert_array_equal(bits(a), bits(b))

        c = child.copy(); c[2, 2] = [6, 0]
        refused(lambda: ctx.trees_grad(c, blen), 'tree 2, row 2')            # a leaf used twice
        c2 = child.copy(); c2[2, 3] = [5, -1]
        refused(lambda: ctx.trees_grad(c2, blen), 'tree 2, row 3')           # no child at all
        for v in (np.nan, -1e-9, np.inf):
            b = blen.copy(); b[2, 1, 1] = v
            refused(lambda: ctx.trees_grad(child, b), 'tree 2, row 1')       # a negative (or non-finite) length
        ch, bl = np.ascontiguousarray(child, dtype=np.int32), np.ascontiguousarray(blen)
        ll, gr = np.empty(4), np.empty(blen.shape)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        raw = lambda *a: ctx._check(ctx._lib.phylo_trees_grad(ctx._h, C.c_int(4), p(ch), p(bl), None, *a))
        refused(lambda: raw(None, p(gr), None, None), 'NULL')                # NULL outputs
        refused(lambda: raw(p(ll), None, None, None), 'NULL')
        with pytest.raises(ValueError):
            ctx.trees_grad(child[:, :3], blen[:, :3])


# ---- 5. a tree whose log-likelihood is not finite: NaN derivatives ----------------------------------------------------------
def test_nan_rule():
    N, S = 5, 70
    g = alignment(N, S, 22, generic=True)
    g[2, 66] = 0.0                                                       # a generic leaf row of zeros kills the site in every tree
    child, blen = random_trees(N, 4, 3)
    with make_ctx(g, gtr_Q()) as ctx:
        ll, grad, curv = ctx.trees_grad(child, blen, prior=PI, want_curv=True)
        assert (ll == -np.inf).all() and np.isnan(grad).all() and np.isnan(curv).all()
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PI)))


# ---- 6. the optimiser on the device -----------------------------------------------------------------------------------------
def nni_neighbours(child):
    """the trees one nearest-neighbour interchange away from child (those whose rows stay children-first)"""
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


def opt_case(N, S, n, seed, Q, pi):
    """an alignment simulated along a tree; that tree and neighbours of it, lengths off by factors in [1/2, 2]"""
    rng = np.random.default_rng(seed)
    c0, b0 = random_rows(N, rng, zeros=False)
    g = simulate(c0, b0 + 0.05, Q, pi, S, rng)
    near = nni_neighbours(c0)
    pool, seen = [], set()
    for c in [c0] + near + nni_neighbours(near[0]):        # the tree, its neighbours, and neighbours of one of them
        if c.tobytes() not in seen:
            seen.add(c.tobytes())
            pool.append(c)
    child = np.array(pool[:n])
    blen = b0[None] * rng.uniform(0.5, 2.0, size=(child.shape[0], N - 1, 2))
    return g, child, blen


def test_optimize_branches_on_the_device():
    N, S = 12, 130
    Q = gtr_Q()
    g, child, blen = opt_case(N, S, 16, 12, Q, PRIOR)
    assert child.shape[0] == 16
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        out = optimize_branches(lambda b: ctx.trees_grad(child, b, want_curv=True), child, blen, max_iter=100)
        print("iterations", out['iterations'], "worst free |g|", np.abs(out['grad'][out['blen'] > 1e-8]).max())
        assert (np.diff(out['history'], axis=0) >= 0).all()                # monotone, tree by tree
        assert out['converged'].all()
        ll, grad = ctx.trees_grad(child, out['blen'])                     # the final gradient, once more from the device
        free = ~((out['blen'] <= 1e-8) & (grad < 0))
        assert (np.abs(grad[free]) <= 1e-6).all()
        assert (ll >= ctx.trees_loglik(child, blen)).all()


# ---- 7. the runner ----------------------------------------------------------------------------------------------------------
def test_runner_score_opt():
    d = load_dataset('primate_data_wang')
    taxa = [str(t) for t in d['taxa']]
    N = len(taxa)
    child, blen = random_trees(N, 12, 3)
    blen = blen + 0.02
    argv = ['--dataset', 'primate_data_wang', '--n_particles', '16', '--num_epoch', '1', '--batch_size', '512', '--jcmodel', 'true',
            '--seed', '2', '--score_opt', 'true', '--tree_tests', '200:1']

    def run(newicks, tmp):
        path = os.path.join(tmp, 'trees.nwk')
        with open(path, 'w') as f:
            f.write('\n'.join(newicks) + '\n')
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'runner.py')] + argv + ['--score_trees', path], cwd=tmp,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        (res,) = glob.glob(os.path.join(tmp, 'results', '*', '*', '*', '*', 'tree_scores.json'))
        here = os.path.dirname(res)
        with open(res) as f:
            scores = json.load(f)
        with open(os.path.join(here, 'trees_ml.nwk')) as f:
            ml = [line.strip() for line in f if line.strip()]
        with open(os.path.join(here, 'tree_tests.json')) as f:
            tests = json.load(f)
        return scores, ml, tests

    with tempfile.TemporaryDirectory() as tmp:
        scores, ml, tests = run([TP.rows_to_newick(c, b, taxa) for c, b in zip(child, blen)], tmp)
    assert len(ml) == 3 and len(scores['trees']) == 3 and tests
    for t in scores['trees']:
        assert t['loglik_ml'] >= t['loglik'] and t['iterations'] >= 1 and isinstance(t['converged'], bool)
    with tempfile.TemporaryDirectory() as tmp:                           # trees given at their ML lengths come back as they are
        again, _, _ = run(ml, tmp)
    for a, b in zip(again['trees'], scores['trees']):
        assert a['loglik'] == pytest.approx(b['loglik_ml'], rel=1e-9)
        assert a['loglik_ml'] == pytest.approx(b['loglik_ml'], rel=1e-9)
