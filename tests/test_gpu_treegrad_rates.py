"""phylo_trees_grad_rates on the device: the derivatives of the mixture log-likelihood of a set of trees
with respect to every branch length, every category's rate and every category's weight.  loglik is held to
phylo_trees_loglik_rates' bits; grad, curv, drate and dweight to the NumPy restatement (treegrad_rates_ref.py, fed with the
device's own branch matrices) within TOL_RATES (scale + |value|), TOL_RATES = 8 E_REF_RATES 2^-53 with E_REF_RATES the
restatement's own error against 50-digit arithmetic (treegrad_rates_cases.py) -- a bound set before the kernel ran.  Then: the
bits of repeated, chunked, reversed, shared and per-tree calls; more work items than workgroups; the NaN rule; what the call
leaves alone; refusals; optimize_rates on the device; runner.py --score_fit.

Every test here needs Context.trees_grad_rates: AttributeError without it."""
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import treegrad_rates_ref as TRR
import trees_edges_cases as EC
from oracle import cpu_ref as O
from phylo_amd import _ffi, model
from phylo_amd import rates as R
from phylo_amd import treepost as TP
from phylo_amd.datasets import load_dataset
from test_gpu_trees_loglik import PI, alignment, bits, gtr_Q, make_ctx, random_trees
from treegrad_rates_cases import MIX_I_G4, TOL_RATES, large_case, fit_case

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PRIOR = np.array([0.1, 0.2, 0.3, 0.4])

MODELS = {
    'C1': (np.array([1.3]), np.array([0.9])),
    'C2': R.rate_model(0.5, 2),
    'C5': MIX_I_G4,                                          # +I+G4: a rate-0 category of weight 0.1
    'C16': R.rate_model(0.7, 15, 0.05),
    'C3-weight0': (np.array([0.2, 1.0, 2.5]), np.array([0.5, 0.0, 0.5])),
}


def case(N, S, **kw):
    return dict(N=N, S=S, **kw)


CASES = {
    'N2-S130': case(2, 130, tile=64), 'N3-S65': case(3, 65, tile=64), 'N5-S64': case(5, 64, tile=64), 'N12-S130': case(12, 130, tile=64),
    'N12-S1': case(12, 1), 'gaps-N12-S65': case(12, 65, tile=64, gaps=True), 'generic-N5-S130': case(5, 130, tile=64, generic=True),
    'jc69-N12-S130': case(12, 130, tile=64, jc=True),
}
RUNS = [(name, 'C5') for name in CASES] + [('N12-S130', m) for m in MODELS if m != 'C5'] + \
    [('N2-S130', 'C16'), ('gaps-N12-S65', 'C3-weight0'), ('generic-N5-S130', 'C2'), ('N12-S1', 'C16')]
T = 7


def same_bits(got, want, what):
    for a, b in zip(got, want):
        np.testing.assert_array_equal(bits(a), bits(b), err_msg=what)


def reference(ctx, child, blen, Q, prior, g, rates, weights):
    """the restatement on the device's own matrices (ctx.expm_batched of rate * blen, the host's one multiply): expm differences
    stay out of the comparison.  rates and weights [C] or [T][C]."""
    rates = np.asarray(rates, dtype=np.float64)
    n = child.shape[0]
    rt = rates if rates.ndim == 2 else np.broadcast_to(rates, (n, rates.size))
    M = np.array([[ctx.expm_batched((rt[t, c] * blen[t]).reshape(-1)).reshape(blen[t].shape + (4, 4)) for c in range(rt.shape[1])]
                  for t in range(n)])
    return TRR.trees_grad_rates(child, M, Q, prior, g, blen, rates, weights)


def close(name, got, ref, scale):
    with np.errstate(invalid='ignore'):
        err = np.abs(got - ref) / (scale + np.abs(ref))
    err = np.where((scale + np.abs(ref)) == 0, np.where(got == 0, 0.0, np.inf), err)       # (a rate sum that is exactly 0: S = 1, zero lengths)
    print("%s: worst |device - reference| / (scale + |value|) = %.3g (TOL_RATES %.3g)" % (name, np.nanmax(err), TOL_RATES))
    assert np.isfinite(got).all(), name
    assert (err <= TOL_RATES).all(), (name, float(np.nanmax(err)), TOL_RATES)


def close_all(name, got, ref):
    """got = (loglik, grad, curv, drate, dweight) of the device, ref the restatement's dict"""
    np.testing.assert_allclose(got[0], ref['loglik'], rtol=1e-12, atol=0)
    close(name + " grad", got[1], ref['grad'], ref['scale'])
    close(name + " curv", got[2], ref['curv'], ref['scale'])
    close(name + " drate", got[3], ref['drate'], ref['drate_scale'])
    close(name + " dweight", got[4], ref['dweight'], ref['dweight'])


# ---- 1. against the reference, several chunks each ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mname", RUNS, ids=['%s-%s' % r for r in RUNS])
def test_against_the_reference(name, mname, monkeypatch):
    kw = CASES[name]
    N, S, jc = kw['N'], kw['S'], kw.get('jc', False)
    rates, weights = MODELS[mname]
    nc = rates.size
    g = alignment(N, S, 100 + N + S, kw.get('gaps', False), kw.get('generic', False))
    Q = O.jc_Q() if jc else gtr_Q()
    child, blen = random_trees(N, 5, T)
    if N > 2:
        assert (blen == 0).any()                                          # trees with zero-length branches
    monkeypatch.setenv('PHYLO_TREES_CHUNK', '3')                          # read when the context is created: three chunks
    with make_ctx(g, Q, jc=jc, tile=kw.get('tile')) as ctx:
        if 'tile' in kw:
            assert ctx.site_tile() == 64
        got = ctx.trees_grad_rates(child, blen, rates, weights, prior=PRIOR, want_curv=True, want_params=True)
        st = ctx.last_trees_stats
        assert st['units'] == T * S * (N - 1) * nc and st['sweep_ms'] > 0
        assert st['n_launches'] == 3 * (5 if kw.get('generic') else 6)    # coded leaves: the gap rows of M too
        same_bits([got[0]], [ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR)], "loglik against phylo_trees_loglik_rates")
        assert np.isfinite(got[0]).all()
        ref = reference(ctx, child, blen, Q, PRIOR, g, rates, weights)
        if mname == 'C5':
            assert (ref['f'][:, 0] == 0).any() or S == 1                  # the invariant class at a variable site
        close_all("%s %s" % (name, mname), got, ref)


@pytest.mark.parametrize("generic", [False, True], ids=['coded', 'generic'])
def test_degenerate_mixtures_against_the_plain_gradient(generic):
    """one category of rate 1 and weight 1, and two of rate 1 and weight 1/2, are phylo_trees_grad's function: held to its
    values within TOL_RATES (the reference's scale); whether the bits agree is printed, not asserted"""
    N, S = 12, 130
    g = alignment(N, S, 51, gaps=True, generic=generic)
    Q = gtr_Q()
    child, blen = random_trees(N, 6, 5)
    with make_ctx(g, Q, tile=64) as ctx:
        ll, grad, curv = ctx.trees_grad(child, blen, prior=PRIOR, want_curv=True)
        for rates, weights in (([1.0], [1.0]), ([1.0, 1.0], [0.5, 0.5])):
            got = ctx.trees_grad_rates(child, blen, rates, weights, prior=PRIOR, want_curv=True, want_params=True)
            ref = reference(ctx, child, blen, Q, PRIOR, g, rates, weights)
            same_bits([got[0]], [ll], "loglik")
            print("C = %d: grad bits %s, curv bits %s those of phylo_trees_grad" % (len(rates), "ARE" if np.array_equal(bits(got[1]), bits(grad))
                                                                                     else "are NOT", "ARE" if np.array_equal(bits(got[2]), bits(curv)) else "are NOT"))
            close("C = %d grad against trees_grad" % len(rates), got[1], grad, ref['scale'])
            close("C = %d curv against trees_grad" % len(rates), got[2], curv, ref['scale'])
            # d/d rate of a single rate-1 class is sum_b blen_b grad_b; d/d weight of weight-w classes sums to S / w ... per class S
            close("C = %d dweight" % len(rates), got[4], ref['dweight'], ref['dweight'])
            close("C = %d drate" % len(rates), got[3], ref['drate'], ref['drate_scale'])


def test_prior_none_is_the_models_pi():
    g = alignment(7, 70, 3, gaps=True)
    pi = np.array([0.4, 0.3, 0.2, 0.1])
    child, blen = random_trees(7, 9, 5)
    rates, weights = MIX_I_G4
    with make_ctx(g, gtr_Q(), pi=pi) as ctx:
        a = ctx.trees_grad_rates(child, blen, rates, weights, want_curv=True, want_params=True)
        b = ctx.trees_grad_rates(child, blen, rates, weights, prior=pi, want_curv=True, want_params=True)
        same_bits(a, b, "prior None")
        assert not np.array_equal(a[1], ctx.trees_grad_rates(child, blen, rates, weights, prior=PI)[1])


# ---- 2. bits ------------------------------------------------------------------------------------------------------------------
def test_calls_chunks_place_and_outputs_give_the_same_bits(monkeypatch):
    N, S, n = 12, 130, 11
    g = alignment(N, S, 31, gaps=True)
    child, blen = random_trees(N, 6, n)
    rates, weights = MIX_I_G4
    kw = dict(prior=PRIOR, want_curv=True, want_params=True)
    got = {}
    for chunk in ('0', '5', '1'):
        monkeypatch.setenv('PHYLO_TREES_CHUNK', chunk)
        with make_ctx(g, gtr_Q(), tile=64) as ctx:
            got[chunk] = ctx.trees_grad_rates(child, blen, rates, weights, **kw)
            assert ctx.last_trees_stats['n_launches'] == 6 * {'0': 1, '5': 3, '1': 11}[chunk]
            same_bits(ctx.trees_grad_rates(child, blen, rates, weights, **kw), got[chunk], "the call again")
            if chunk == '5':
                rev = ctx.trees_grad_rates(child[::-1], blen[::-1], rates, weights, **kw)
                same_bits([a[::-1] for a in rev], got[chunk], "the set reversed")
                full = got[chunk]
                same_bits(ctx.trees_grad_rates(child, blen, rates, weights, prior=PRIOR), full[:2], "grad alone")
                same_bits(ctx.trees_grad_rates(child, blen, rates, weights, prior=PRIOR, want_curv=True), full[:3], "grad and curv")
                only = ctx.trees_grad_rates(child, blen, rates, weights, prior=PRIOR, want_params=True)
                same_bits(only, (full[0], full[1], full[3], full[4]), "grad and params")
                # a mixture per tree: equal rows are the shared call; different rows are tree t of the shared call with row t
                tiled = ctx.trees_grad_rates(child, blen, np.tile(rates, (n, 1)), np.tile(weights, (n, 1)), **kw)
                same_bits(tiled, full, "per-tree rows all equal")
                rng = np.random.default_rng(8)
                rt = np.array([R.rate_model(a, 4, p)[0] for a, p in zip(rng.uniform(0.2, 3.0, n), rng.uniform(0.01, 0.4, n))])
                wt = np.array([R.rate_model(1.0, 4, p)[1] for p in rng.uniform(0.01, 0.4, n)])
                own = ctx.trees_grad_rates(child, blen, rt, wt, **kw)
                for t in range(n):
                    shared = ctx.trees_grad_rates(child, blen, rt[t], wt[t], **kw)
                    same_bits([a[t] for a in own], [a[t] for a in shared], "tree %d under its own row" % t)
                same_bits([own[0]], [np.array([ctx.trees_loglik_rates(child[t], blen[t], rt[t], wt[t], prior=PRIOR)[0] for t in range(n)])],
                          "per-tree loglik against phylo_trees_loglik_rates")
    for chunk in ('5', '1'):
        same_bits(got[chunk], got['0'], "chunks of " + chunk)


# ---- 3. more items than workgroups ----------------------------------------------------------------------------------------------
def test_strided_items_five_taxa(monkeypatch):
    from test_gpu_trees_edges import compute_units
    cus = compute_units()
    n = -(-(8 * cus + 5) // 3)                                            # 3 tiles: at least 8 CUs + 5 items
    g, child, blen, Q = EC.small_strided(n)
    rates, weights = MIX_I_G4
    kw = dict(prior=PRIOR, want_curv=True, want_params=True)
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        assert -(-g.shape[1] // ctx.site_tile()) == 3
        cap = min(8 * cus, (256 << 20) // (rates.size * 4 * 2 * 2048))   # ptgr_make_plan's grid, the items apart
        assert cap == 8 * cus and 3 * n >= cap + 5
        full = ctx.trees_grad_rates(child, blen, rates, weights, **kw)
        assert ctx.last_trees_stats['n_launches'] == 6                   # one chunk: items > grid, workgroups stride
        sample = sorted(set(range(4)) | set(range(cap // 3 - 1, min(n, cap // 3 + 3))) | {n - 1})
        ref = reference(ctx, child[sample], blen[sample], Q, PRIOR, g, rates, weights)
        close_all("N5 strided", [a[sample] for a in full], ref)
    monkeypatch.setenv('PHYLO_TREES_CHUNK', '1')
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        same_bits(ctx.trees_grad_rates(child, blen, rates, weights, **kw), full, "strided against one tree per chunk")


def test_strided_items_512_taxa_16_categories(monkeypatch):
    """N = 512 under 16 categories: 32 MiB of node store per workgroup, so 8 workgroups for 11 trees' items; 60 KiB of LDS"""
    g, child, blen, Q, rates, weights = large_case()
    n = child.shape[0]
    assert rates.size == 16 and n == 11 and (256 << 20) // (16 * 511 * 2 * 2048) == 8
    kw = dict(prior=PRIOR, want_curv=True, want_params=True)
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        full = ctx.trees_grad_rates(child, blen, rates, weights, **kw)
        assert ctx.last_trees_stats['n_launches'] == 2 * 6 and 9 * -(-g.shape[1] // ctx.site_tile()) > 8      # chunks of 9 trees (64 MiB)
        same_bits([full[0]], [ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR)], "loglik against phylo_trees_loglik_rates")
        sample = [0, 9]                                                   # a first item and a second item of a workgroup
        ref = reference(ctx, child[sample], blen[sample], Q, PRIOR, g, rates, weights)
        assert (ref['m'] > EC.ROOMY).all()
        close_all("N512 C16", [a[sample] for a in full], ref)
    monkeypatch.setenv('PHYLO_TREES_CHUNK', '1')
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        same_bits(ctx.trees_grad_rates(child, blen, rates, weights, **kw), full, "strided against one tree per chunk")


# ---- 4. the NaN rule ------------------------------------------------------------------------------------------------------------
def test_nan_rule():
    N, S = 5, 70
    g = alignment(N, S, 22, generic=True)
    g[2, 66] = 0.0                                                       # a generic leaf row of zeros kills the site in every tree and category
    child, blen = random_trees(N, 4, 3)
    rates, weights = MIX_I_G4
    with make_ctx(g, gtr_Q()) as ctx:
        got = ctx.trees_grad_rates(child, blen, rates, weights, prior=PI, want_curv=True, want_params=True)
        assert (got[0] == -np.inf).all()
        for a in got[1:]:
            assert np.isnan(a).all()
        same_bits([got[0]], [ctx.trees_loglik_rates(child, blen, rates, weights, prior=PI)], "loglik")


def test_invariant_class_at_variable_sites_is_finite():
    N, S = 8, 130
    g = alignment(N, S, 23)                                              # coded, no gaps: the sites are variable ...
    g[:, ::7] = g[0, ::7]                                                # ... but every seventh, a constant column
    child, blen = random_trees(N, 4, 5)
    rates, weights = MIX_I_G4
    with make_ctx(g, gtr_Q(), tile=64) as ctx:
        got = ctx.trees_grad_rates(child, blen, rates, weights, prior=PI, want_curv=True, want_params=True)
        _, cats = ctx.trees_loglik_rates(child, blen, rates, weights, prior=PI, want_cats=True)
        assert (cats[:, 0] == 0).any() and (cats[:, 0] > 0).any()         # f_0 = 0 at variable sites, > 0 at constant ones
        for a in got:
            assert np.isfinite(a).all()


# ---- 5. what the call leaves alone, and refusals ----------------------------------------------------------------------------------
def test_sweep_backward_summary_and_scratch_are_left_alone():
    g = load_dataset('primate_data')['genome'][:6, 100:170].copy()
    N, S, K, seed = 6, 70, 64, 5
    pi = np.array([[0.3, 0.2, 0.2, 0.3]])
    Q = model.get_Q(model.init_y_q())
    lam = np.linspace(5.0, 15.0, N - 1)
    rates, weights = MIX_I_G4
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, pi, lam, lam[::-1].copy())
        out = ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        grad = ctx.sweep_backward()
        ctx.sweep_async(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        child, blen = TP.particle_trees(out['merges'], out['ancestors'], out['left_branches'], out['right_branches'], seed=seed)
        ll, sites = ctx.trees_loglik(child[:7], blen[:7], want_sites=True)
        rll, rsites = ctx.trees_loglik_rates(child[:7], blen[:7], rates, weights, want_sites=True)
        rl = ctx.rell(sites, 50, 3, want_reps=True)
        plain = ctx.trees_grad(child[:7], blen[:7], want_curv=True)
        got = ctx.trees_grad_rates(child, blen, rates, weights, want_curv=True, want_params=True)   # between a sweep and its pending reverse pass
        for a in got:
            assert np.isfinite(a).all()
        same_bits([got[0][:7]], [rll], "loglik")
        grad2 = ctx.sweep_backward()
        again = ctx.sweep_fetch()
        for key in ('log_weights', 'log_likelihood', 'left_branches', 'right_branches'):
            np.testing.assert_array_equal(bits(again[key]), bits(out[key]), err_msg=key)
        np.testing.assert_array_equal(again['ancestors'], out['ancestors'])
        assert bits(again['logZ']) == bits(out['logZ'])
        for key in ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q'):
            np.testing.assert_array_equal(bits(grad2[key]), bits(grad[key]), err_msg=key)
        # the scratch of sections 11, 11b, 12 and 13: the same calls give the same bits afterwards
        same_bits(ctx.trees_loglik(child[:7], blen[:7], want_sites=True), (ll, sites), "section 11")
        same_bits(ctx.trees_loglik_rates(child[:7], blen[:7], rates, weights, want_sites=True), (rll, rsites), "section 11b")
        same_bits([ctx.rell(sites, 50, 3, want_reps=True)['rep_loglik']], [rl['rep_loglik']], "section 12")
        same_bits(ctx.trees_grad(child[:7], blen[:7], want_curv=True), plain, "section 13")
        tab = ctx.tree_summary()                                          # a tree summary made before the call still has its branch pass
        ctx.trees_grad_rates(child[:3], blen[:3], rates, weights)
        tb = ctx.tree_branches(tab)
        assert np.isfinite(tb['leaf_stats']).all()
        third = ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)   # the next sweep's bits
        np.testing.assert_array_equal(bits(third['log_weights']), bits(out['log_weights']))


def test_refusals_queue_nothing():
    N, S = 5, 70
    g = alignment(N, S, 41)
    child, blen = random_trees(N, 8, 4)
    child[2] = np.array([[0, 1], [2, 3], [6, 4], [5, 7]], dtype=np.int32)
    rates, weights = R.rate_model(0.5, 4)
    kw = dict(want_curv=True, want_params=True)
    with _ffi.Context(4, N, S) as ctx:
        with pytest.raises(_ffi.PhyloError) as e:
            ctx.trees_grad_rates(child, blen, rates, weights)
        assert e.value.code == -6
        ctx.set_leaves(g)
        ctx.set_model(gtr_Q(), PI, np.full(N - 1, 10.0), np.full(N - 1, 10.0))
        ref = ctx.trees_grad_rates(child, blen, rates, weights, **kw)

        def refused(call, *what):
            with pytest.raises(_ffi.PhyloError) as e:
                call()
            assert e.value.code == -1, str(e.value)
            for x in what:
                assert x in str(e.value), str(e.value)
            same_bits(ctx.trees_grad_rates(child, blen, rates, weights, **kw), ref, "a valid call afterwards")

        c = child.copy(); c[2, 2] = [6, 0]
        refused(lambda: ctx.trees_grad_rates(c, blen, rates, weights), 'tree 2, row 2', 'twice')
        c2 = child.copy(); c2[2, 3] = [5, -1]
        refused(lambda: ctx.trees_grad_rates(c2, blen, rates, weights), 'tree 2, row 3')
        for v in (np.nan, -1e-9, np.inf):
            b = blen.copy(); b[2, 1, 1] = v
            refused(lambda: ctx.trees_grad_rates(child, b, rates, weights), 'tree 2, row 1')
        refused(lambda: ctx.trees_grad_rates(child, blen, [], []), 'C=0')
        refused(lambda: ctx.trees_grad_rates(child, blen, np.ones(17), np.full(17, 1 / 17)), 'C=17')
        rt, wt = np.tile(rates, (4, 1)), np.tile(weights, (4, 1))
        for v in (-1e-9, np.nan, np.inf, -np.inf):
            r = rates.copy(); r[2] = v
            refused(lambda: ctx.trees_grad_rates(child, blen, r, weights), 'rate', 'category 2')
            w = weights.copy(); w[1] = v
            refused(lambda: ctx.trees_grad_rates(child, blen, rates, w), 'weight', 'category 1')
            r = rt.copy(); r[3, 2] = v                                    # under per_tree the message names the tree
            refused(lambda: ctx.trees_grad_rates(child, blen, r, wt), 'tree 3', 'rate', 'category 2')
            w = wt.copy(); w[1, 0] = v
            refused(lambda: ctx.trees_grad_rates(child, blen, rt, w), 'tree 1', 'weight', 'category 0')
        b = blen.copy(); b[1, 3, 0] = 1e308
        refused(lambda: ctx.trees_grad_rates(child, b, [0.5, 1.0, 10.0], [0.3, 0.3, 0.4]), 'tree 1', 'row 3, category 2')
        ch, bl = np.ascontiguousarray(child, dtype=np.int32), np.ascontiguousarray(blen)
        ll, gr = np.empty(4), np.empty(blen.shape)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        raw = lambda *a: ctx._check(ctx._lib.phylo_trees_grad_rates(ctx._h, C.c_int(4), *a))
        full = (p(ch), p(bl), C.c_int(4), p(rates), p(weights), C.c_int(0), None, p(ll), p(gr), None, None, None, None)
        for k in (0, 1, 3, 4, 7, 8):                                      # child, blen, rate, weight, loglik, grad
            args = list(full); args[k] = None
            refused(lambda: raw(*args), 'NULL')
        args = list(full); args[5] = C.c_int(2)
        refused(lambda: raw(*args), 'per_tree')
        raw(*full)                                                        # curv, drate, dweight and perf may be NULL
        same_bits([ll, gr], ref[:2], "the raw call")
        with pytest.raises(ValueError):
            ctx.trees_grad_rates(child, blen, rates, weights[:3])
        with pytest.raises(ValueError):
            ctx.trees_grad_rates(child, blen, rt[:3], wt[:3])
        with pytest.raises(ValueError):
            ctx.trees_grad_rates(child[:, :3], blen[:, :3], rates, weights)


# ---- 6. optimize_rates on the device ------------------------------------------------------------------------------------------
def test_optimize_rates_on_the_device():
    from phylo_amd.treeopt import optimize_rates
    N, S, C = 8, 260, 4
    Q = gtr_Q()
    g, child, blen = fit_case(N, S, 6, 21, Q, PRIOR)
    assert child.shape[0] == 6
    gtol = 1e-6
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        calls = [0]

        def fn(b, r, w):
            calls[0] += 1
            return ctx.trees_grad_rates(child, b, r, w, want_curv=True, want_params=True)

        r0, w0 = R.rate_model(1.0, C)
        start = ctx.trees_loglik_rates(child, blen, r0, w0)
        out = optimize_rates(fn, child, blen, 1.0, C, gtol=gtol)
        print("iterations", out['iterations'], "alpha", out['alpha'], "device calls", calls[0])
        assert calls[0] == out['history'].shape[0]                        # one device call per iteration
        assert (np.diff(out['history'], axis=0) >= 0).all()               # monotone, tree by tree
        assert out['converged'].all()
        assert (out['alpha'] >= 0.02).all() and (out['alpha'] <= 100.0).all()
        ll, grad, drate, dweight = ctx.trees_grad_rates(child, out['blen'], out['rates'], out['weights'], want_params=True)   # once more from the device
        free = ~((out['blen'] <= 1e-8) & (grad < 0))
        assert (np.abs(grad[free]) <= gtol).all()
        jac = [R.rate_model_jacobian(a, C) for a in out['alpha']]
        da, _ = R.chain(drate, dweight, (np.array([j[0] for j in jac]), np.array([j[1] for j in jac])))
        at_bound = (out['alpha'] <= 0.02) | (out['alpha'] >= 100.0)
        assert (np.abs(da * out['alpha'])[~at_bound] <= gtol).all()       # the gradient in log alpha
        assert (ll >= start).all()
        np.testing.assert_allclose(ll, out['loglik'], rtol=2.0 ** -46, atol=0)   # (of two values that close the optimiser keeps the larger)


# ---- 7. the runner --------------------------------------------------------------------------------------------------------------
def test_runner_score_fit():
    d = load_dataset('primate_data_wang')
    taxa = [str(t) for t in d['taxa']]
    N = len(taxa)
    child, blen = random_trees(N, 12, 3)
    blen = blen + 0.02
    argv = ['--dataset', 'primate_data_wang', '--n_particles', '16', '--num_epoch', '1', '--batch_size', '512', '--jcmodel', 'true',
            '--seed', '2']

    def run(newicks, extra, tmp):
        path = os.path.join(tmp, 'trees.nwk')
        with open(path, 'w') as f:
            f.write('\n'.join(newicks) + '\n')
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'runner.py')] + argv + ['--score_trees', path] + extra, cwd=tmp,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        (res,) = glob.glob(os.path.join(tmp, 'results', '*', '*', '*', '*', 'tree_scores.json'))
        with open(res) as f:
            return json.load(f), os.path.dirname(res)

    with tempfile.TemporaryDirectory() as tmp:
        scores, here = run([TP.rows_to_newick(c, b, taxa) for c, b in zip(child, blen)],
                           ['--score_rates', 'gamma:1.0:4', '--score_fit', 'branches+alpha', '--tree_tests', '200:1'], tmp)
        with open(os.path.join(here, 'trees_ml.nwk')) as f:
            ml = [line.strip() for line in f if line.strip()]
        with open(os.path.join(here, 'tree_tests.json')) as f:
            tests = json.load(f)
        with open(os.path.join(here, 'run_parameters.txt')) as f:
            assert 'score_fit : branches+alpha' in f.read()
    assert len(ml) == 3 and len(scores['trees']) == 3 and tests and scores['rates']['spec'] == 'gamma:1.0:4'
    for t in scores['trees']:
        assert t['loglik_ml'] >= t['loglik'] and t['iterations'] >= 1 and isinstance(t['converged'], bool)
        assert 0.02 <= t['alpha'] <= 100.0 and 'pinv' not in t
    np.testing.assert_allclose(tests['obs'], [t['loglik_ml'] for t in scores['trees']], rtol=1e-12)   # the tests saw the fitted factors
    with tempfile.TemporaryDirectory() as tmp:                           # tree 1 at its ML lengths under its fitted alpha comes back as it is
        again, _ = run(ml, ['--score_rates', 'gamma:%r:4' % scores['trees'][1]['alpha']], tmp)
    assert again['trees'][1]['loglik'] == pytest.approx(scores['trees'][1]['loglik_ml'], rel=1e-9)
    assert 'loglik_ml' not in again['trees'][1]
