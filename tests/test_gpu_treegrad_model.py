"""phylo_trees_grad_model on the device: the derivatives of the log-likelihood of a set of trees along
directions of the generator and with respect to the root distribution.  loglik is held to phylo_trees_loglik's bits and grad to
phylo_trees_grad's; dtheta and dprior to the NumPy restatement (treegrad_model_ref.py, fed with the device's own branch matrices
and its own restated Frechet derivatives) within TOL_MODEL (scale + |value|), TOL_MODEL = 8 E_REF_MODEL 2^-53 with E_REF_MODEL
the restatement's own error against 50-digit arithmetic -- a bound set before the kernel ran.  Then: what changes no bit, more
items than workgroups, 512 taxa at 16 directions, identities that need no reference, the NaN rule, refusals, what the call
leaves alone.

Every test here needs Context.trees_grad_model: AttributeError without it."""
import ctypes as C

import numpy as np
import pytest

import treegrad_model_ref as MR
import treegrad_ref as TR
import trees_edges_cases as EC
from oracle import cpu_ref as O
from phylo_amd import _ffi, model, modelfit
from phylo_amd import treepost as TP
from phylo_amd.datasets import load_dataset
from test_gpu_trees_edges import compute_units
from test_gpu_trees_loglik import PI, alignment, bits, gtr_Q, make_ctx, random_trees, shaped_trees
from treegrad_cases import TOL
from treegrad_model_ref import TOL_MODEL
from trees_cases import balanced_rows, caterpillar_rows

pytestmark = pytest.mark.gpu
PRIOR = np.array([0.1, 0.2, 0.3, 0.4])


def directions(P, Q, seed=1):
    """P directions: the twelve of the row-softmax (of a random y_q), Q itself, random ones"""
    rng = np.random.default_rng(seed)
    d = np.concatenate([modelfit.q_directions(rng.normal(size=(4, 4))), Q[None], rng.normal(size=(3, 4, 4))])
    return np.ascontiguousarray({1: d[5:6], 12: d[:12], 16: d}[P])


def reference(ctx, child, blen, Q, dirs, prior, g, jc=False, tile=None):
    """the restatement on the device's own branch matrices (ctx.expm_batched): expm differences stay out of the comparison"""
    M = ctx.expm_batched(blen.reshape(-1)).reshape(blen.shape + (4, 4))
    D = MR.direction_matrices(Q, dirs, blen, jc=jc)
    return MR.trees_grad_model(child, M, D, prior, g, tile=tile)


def close(name, got, ref, scale, tol=TOL_MODEL):
    err = np.abs(got - ref) / (scale + np.abs(ref))
    print("%s: worst |device - reference| / (scale + |value|) = %.3g (tolerance %.3g)" % (name, np.nanmax(err), tol))
    assert np.isfinite(got).all(), name
    assert (err <= tol).all(), (name, float(np.nanmax(err)), tol)


def same(a, b, what=""):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(bits(x), bits(y), err_msg=what)


def case(N, S, P=12, **kw):
    return dict(N=N, S=S, P=P, **kw)


CASES = {
    'N2': case(2, 130), 'N3': case(3, 130), 'N5': case(5, 130), 'N12': case(12, 130),
    'S1': case(5, 1), 'S63': case(5, 63), 'S64': case(5, 64), 'S65': case(5, 65),
    'gaps': case(12, 130, gaps=True), 'generic': case(12, 130, generic=True), 'jc69': case(12, 130, jc=True, gaps=True),
    'caterpillar': case(12, 65, shape=caterpillar_rows), 'balanced': case(12, 65, shape=balanced_rows, gaps=True),
    'P1': case(5, 130, P=1, gaps=True), 'P16': case(5, 130, P=16, gaps=True),
    # the default tile: one item of three strips of 128 sites (the last with 44 live lanes in its first step, none in its second),
    # so the lane accumulators of dtheta and dprior are carried from strip to strip; and S = 600, a half-full second step
    'S300-strips': case(5, 300, gaps=True, tile=None), 'S600-strips-N12': case(12, 600, P=16, gaps=True, tile=None),
}
NT = 5


# ---- 1. against the restatement, three chunks each; and what changes no bit -------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_reference(name, monkeypatch):
    kw = CASES[name]
    N, S, P, jc = kw['N'], kw['S'], kw['P'], kw.get('jc', False)
    g = alignment(N, S, 100 + N + S, kw.get('gaps', False), kw.get('generic', False))
    Q = O.jc_Q() if jc else gtr_Q()
    child, blen = shaped_trees(kw['shape'], N, 5, NT) if 'shape' in kw else random_trees(N, 5, NT)
    if N > 2:
        assert (blen == 0).any()                                          # trees with zero-length branches
    dirs = directions(P, Q)
    monkeypatch.setenv('PHYLO_TREES_CHUNK', '2')                          # read when the context is created: three chunks
    with make_ctx(g, Q, jc=jc, tile=kw.get('tile', 64)) as ctx:
        tile = ctx.site_tile()
        assert tile == 64 if 'tile' not in kw else tile >= S              # the default tile: one item, ceil(S / 128) strips
        ll, dth, grad, dpr = ctx.trees_grad_model(child, blen, dirs, prior=PRIOR, want_grad=True)
        st = ctx.last_trees_stats
        assert st['units'] == NT * S * (N - 1) * (1 + P) and st['sweep_ms'] > 0
        assert st['n_launches'] == 3 * (7 if kw.get('generic') else 8)    # coded leaves: the gap rows of M too
        assert dth.shape == (NT, P) and dpr.shape == (NT, 4) and grad.shape == blen.shape
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)), err_msg="loglik against phylo_trees_loglik")
        np.testing.assert_array_equal(bits(grad), bits(ctx.trees_grad(child, blen, prior=PRIOR)[1]), err_msg="grad against phylo_trees_grad")
        assert np.isfinite(ll).all()
        same(ctx.trees_grad_model(child, blen, dirs, prior=PRIOR, want_grad=True), (ll, dth, grad, dpr), "a repeated call")
        same(ctx.trees_grad_model(child, blen, dirs, prior=PRIOR), (ll, dth, dpr), "without grad")
        assert ctx.last_trees_stats['n_launches'] == 3 * (5 if kw.get('generic') else 6)
        same(ctx.trees_grad_model(child, blen, dirs, prior=PRIOR, want_prior=False), (ll, dth), "without dprior")
        same(ctx.trees_grad_model(child, blen, dirs, prior=PRIOR, want_grad=True, want_prior=False), (ll, dth, grad), "without dprior, with grad")
        rev = ctx.trees_grad_model(child[::-1], blen[::-1], dirs, prior=PRIOR, want_grad=True)   # a tree's bits do not depend on its place
        same([a[::-1] for a in rev], (ll, dth, grad, dpr), "a tree's place")
        rll, rdth, rdpr, sc_t, sc_p = reference(ctx, child, blen, Q, dirs, PRIOR, g, jc=jc, tile=tile)
        np.testing.assert_allclose(ll, rll, rtol=1e-12, atol=0)
        close(name + " dtheta", dth, rdth, sc_t)
        close(name + " dprior", dpr, rdpr, sc_p)


def test_prior_none_is_the_models_pi():
    g = alignment(7, 70, 3, gaps=True)
    pi = np.array([0.4, 0.3, 0.2, 0.1])
    child, blen = random_trees(7, 9, 5)
    Q = gtr_Q()
    dirs = directions(12, Q)
    with make_ctx(g, Q, pi=pi) as ctx:
        a, b = ctx.trees_grad_model(child, blen, dirs, want_grad=True), ctx.trees_grad_model(child, blen, dirs, prior=pi, want_grad=True)
        same(a, b)
        assert not np.array_equal(a[1], ctx.trees_grad_model(child, blen, dirs, prior=PI)[1])


def test_chunks_and_directions_change_no_bit(monkeypatch):
    """chunks of all, five and one tree; and every column of dtheta when its direction is passed alone (P = 1), among 12, or among
    16 in another place"""
    g = alignment(12, 130, 31, gaps=True)
    child, blen = random_trees(12, 6, 11)
    Q = gtr_Q()
    dirs = directions(16, Q)
    got = {}
    for chunk in ('0', '5', '1'):
        monkeypatch.setenv('PHYLO_TREES_CHUNK', chunk)
        with make_ctx(g, Q, tile=64) as ctx:
            got[chunk] = ctx.trees_grad_model(child, blen, dirs, want_grad=True)
            assert ctx.last_trees_stats['n_launches'] == 8 * {'0': 1, '5': 3, '1': 11}[chunk]
            if chunk == '5':
                full = got[chunk][1]
                for p in (0, 7, 12, 15):
                    alone = ctx.trees_grad_model(child, blen, dirs[p:p + 1], want_prior=False)[1]
                    np.testing.assert_array_equal(bits(alone[:, 0]), bits(full[:, p]), err_msg="direction %d alone" % p)
                twelve = ctx.trees_grad_model(child, blen, dirs[:12], want_prior=False)[1]
                np.testing.assert_array_equal(bits(twelve), bits(full[:, :12]))
                turned = ctx.trees_grad_model(child, blen, dirs[::-1], want_prior=False)[1]
                np.testing.assert_array_equal(bits(turned[:, ::-1]), bits(full))
    for chunk in ('5', '1'):
        same(got[chunk], got['0'], "chunks of " + chunk)


# ---- 2. more items than workgroups ------------------------------------------------------------------------------------------
def test_strided_items_five_taxa(monkeypatch):
    """N = 5, three tiles, 8 CUs + 5 items or more in one chunk, so that workgroups take a second item; bit for bit against chunks
    of one item per workgroup, and against the restatement on the first trees and those of the second items"""
    cus = compute_units()
    T = EC.strided_T(5, 3, cus)
    g, child, blen, Q = EC.small_strided(T)
    cap = EC.updown_cap(5, cus)
    assert 3 * T >= cap + 5
    dirs = directions(16, Q)[10:13]                                       # two softmax directions and Q
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        full = ctx.trees_grad_model(child, blen, dirs, prior=PRIOR, want_grad=True)
        assert ctx.last_trees_stats['n_launches'] == 8                    # one chunk: items > grid, workgroups stride
        np.testing.assert_array_equal(bits(full[0]), bits(ctx.trees_loglik(child, blen, prior=PRIOR)))
        sample = sorted(set(range(4)) | set(range(cap // 3 - 2, T)))
        rll, rdth, rdpr, sc_t, sc_p = reference(ctx, child[sample], blen[sample], Q, dirs, PRIOR, g, tile=64)
        close("strided dtheta", full[1][sample], rdth, sc_t)
        close("strided dprior", full[3][sample], rdpr, sc_p)
    chunk = cap // 3
    monkeypatch.setenv('PHYLO_TREES_CHUNK', str(chunk))
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        parts = ctx.trees_grad_model(child, blen, dirs, prior=PRIOR, want_grad=True)
        assert ctx.last_trees_stats['n_launches'] == -(-T // chunk) * 8
    same(full, parts, "strided against one item per workgroup")


# ---- 3. the LDS bound: 512 taxa, 16 directions ------------------------------------------------------------------------------
def test_512_taxa_16_directions():
    g, child, blen, Q = EC.big_case('balanced-N512')
    child, blen = child[:2], blen[:2]
    dirs = directions(16, Q)
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        ll, dth, grad, dpr = ctx.trees_grad_model(child, blen, dirs, prior=PRIOR, want_grad=True)
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)))
        np.testing.assert_array_equal(bits(grad), bits(ctx.trees_grad(child, blen, prior=PRIOR)[1]))
        rll, rdth, rdpr, sc_t, sc_p = reference(ctx, child, blen, Q, dirs, PRIOR, g)
        close("N512 dtheta", dth, rdth, sc_t)
        close("N512 dprior", dpr, rdpr, sc_p)


# ---- 4. identities that need no reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("jc", [False, True], ids=['gtr', 'jc69'])
def test_identities(jc):
    """Each side of an identity is a device sum within its tolerance of the exact value of ITS OWN terms (device against
    restatement 8 E, restatement against exact E: 9/8 of the tolerance), so the two sides meet within the sum of those."""
    N, S = 12, 130
    g = alignment(N, S, 57, gaps=True)
    Q = O.jc_Q() if jc else gtr_Q()
    Qe = MR.JC_Q if jc else Q
    child, blen = random_trees(N, 8, 4)
    rng = np.random.default_rng(4)
    E1, E2 = rng.normal(size=(2, 4, 4))
    dirs = np.stack([Qe, E1, E2, 2 * E1 - 3 * E2])
    with make_ctx(g, Q, jc=jc, tile=64) as ctx:
        ll, dth, grad, dpr = ctx.trees_grad_model(child, blen, dirs, prior=PRIOR, want_grad=True)
        _, _, _, sc_t, sc_p = reference(ctx, child, blen, Q, dirs, PRIOR, g, jc=jc, tile=64)
        M = ctx.expm_batched(blen.reshape(-1)).reshape(blen.shape + (4, 4))
        _, _, _, sc_g = TR.trees_grad(child, M, Qe, PRIOR, g)
    # L_s is linear in the prior: sum_j prior[j] dprior[j] = S
    lhs = (dpr * PRIOR).sum(axis=1)
    bound = 9 / 8 * TOL_MODEL * (PRIOR * (sc_p + np.abs(dpr))).sum(axis=1) + 8 * 2.0 ** -53 * S
    print("sum prior dprior - S:", lhs - S, "bound", bound)
    assert (np.abs(lhs - S) <= bound).all()
    # scaling Q is scaling every length: dtheta along Q_eff = sum_b blen_b grad_b
    rhs = (blen * grad).sum(axis=(1, 2))
    bound = 9 / 8 * (TOL_MODEL * (sc_t[:, 0] + np.abs(dth[:, 0])) + TOL * (blen * (sc_g + np.abs(grad))).sum(axis=(1, 2)))
    print("dtheta along Q - sum blen grad:", dth[:, 0] - rhs, "bound", bound)
    assert (np.abs(dth[:, 0] - rhs) <= bound).all()
    # linearity in the direction
    s = sc_t + np.abs(dth)
    bound = 9 / 8 * TOL_MODEL * (s[:, 3] + 2 * s[:, 1] + 3 * s[:, 2])
    print("linearity:", dth[:, 3] - (2 * dth[:, 1] - 3 * dth[:, 2]), "bound", bound)
    assert (np.abs(dth[:, 3] - (2 * dth[:, 1] - 3 * dth[:, 2])) <= bound).all()


# ---- 5. the NaN rule, and the floor of the range ----------------------------------------------------------------------------
def test_nan_rule():
    N, S = 5, 70
    g = alignment(N, S, 22, generic=True)
    child, blen = random_trees(N, 4, 3)
    blen = blen + 0.01
    Q = gtr_Q()
    dirs = directions(12, Q)
    with make_ctx(g, Q) as ctx:
        clean = ctx.trees_grad_model(child, blen, dirs, prior=PI, want_grad=True)
        assert all(np.isfinite(a).all() for a in clean)
    g0 = g.copy()
    g0[2, 66] = 0.0                                                      # a generic leaf row of zeros kills the site in every tree
    with make_ctx(g0, Q) as ctx:
        ll, dth, grad, dpr = ctx.trees_grad_model(child, blen, dirs, prior=PI, want_grad=True)
        assert (ll == -np.inf).all() and np.isnan(dth).all() and np.isnan(grad).all() and np.isnan(dpr).all()
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PI)))
    # ... and in ONE tree of a set only (a row of zeros spoils every tree): tree 1 joins leaves 0 and 1 by zero-length branches
    # (M = I), and at a site where the two hold different letters their parent has no state left
    gi = alignment(N, S, 22)
    s = int(np.nonzero((gi[0] != gi[1]).any(axis=1) & (gi[0].sum(axis=1) == 1) & (gi[1].sum(axis=1) == 1))[0][0])
    c1 = np.array([[0, 1], [2, 3], [5, 6], [7, 4]], dtype=np.int32)
    child2 = np.stack([child[0], c1, child[2]])
    blen2 = blen.copy()
    blen2[1, 0] = 0.0
    with make_ctx(gi, Q) as ctx:
        ll, dth, grad, dpr = ctx.trees_grad_model(child2, blen2, dirs, prior=PI, want_grad=True)
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child2, blen2, prior=PI)))
        assert ll[1] == -np.inf and np.isnan(dth[1]).all() and np.isnan(grad[1]).all() and np.isnan(dpr[1]).all(), s
        for t in (0, 2):
            assert np.isfinite(ll[t]) and np.isfinite(dth[t]).all() and np.isfinite(grad[t]).all() and np.isfinite(dpr[t]).all()
        alone = ctx.trees_grad_model(child2[[0, 2]], blen2[[0, 2]], dirs, prior=PI, want_grad=True)
        same([a[[0, 2]] for a in (ll, dth, grad, dpr)], alone, "the other trees keep their bits")


def test_scaled_to_the_floor_stays_finite():
    """four sites of every tree scaled by exact powers of two until the smallest factor lies in [2^-1020, 2^-1019): the terms are
    ratios, so the unscaled restatement is the yardstick; dprior's terms x_root / L_s are ratios too"""
    g, child, blen, Q = EC.scaled_base()
    dirs = directions(12, Q)
    at = list(EC.SCALED_SITES)
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        ll0, dth0, dpr0 = ctx.trees_grad_model(child, blen, dirs, prior=PRIOR)
        M = ctx.expm_batched(blen.reshape(-1)).reshape(blen.shape + (4, 4))
        L0 = TR.trees_site_factors(child, M, PRIOR, g)
        _, rdth, rdpr, sc_t, sc_p = reference(ctx, child, blen, Q, dirs, PRIOR, g, tile=64)
    close("unscaled dtheta", dth0, rdth, sc_t)
    e = EC.scaled_exponents('at-the-floor', L0)
    gs = EC.scaled_leaves(g, e)
    with make_ctx(gs, Q, pi=PRIOR, tile=64) as ctx:
        ll, dth, dpr = ctx.trees_grad_model(child, blen, dirs, prior=PRIOR)
        plain, sites = ctx.trees_loglik(child, blen, prior=PRIOR, want_sites=True)
    np.testing.assert_array_equal(bits(ll), bits(plain))
    assert (sites[:, at] >= TR.FLOOR).all() and (sites[:, at] <= 2.0 ** -1000).all() and (sites[:, at].min(axis=0) < 2.0 ** -1019).all()
    assert np.isfinite(ll).all()
    close("at the floor: dtheta against the unscaled restatement", dth, rdth, sc_t)
    close("at the floor: dprior against the unscaled restatement", dpr, rdpr, sc_p)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing():
    N, S = 5, 70
    g = alignment(N, S, 41)
    child, blen = random_trees(N, 8, 4)
    child[2] = np.array([[0, 1], [2, 3], [6, 4], [5, 7]], dtype=np.int32)
    Q = gtr_Q()
    dirs = directions(16, Q)
    with _ffi.Context(4, N, S) as ctx:
        with pytest.raises(_ffi.PhyloError) as e:
            ctx.trees_grad_model(child, blen, dirs)
        assert e.value.code == -6
        ctx.set_leaves(g)
        ctx.set_model(Q, PI, np.full(N - 1, 10.0), np.full(N - 1, 10.0))
        ref = ctx.trees_grad_model(child, blen, dirs, want_grad=True)

        def refused(call, what):
            with pytest.raises(_ffi.PhyloError) as e:
                call()
            assert e.value.code == -1 and what in str(e.value), str(e.value)
            same(ctx.trees_grad_model(child, blen, dirs, want_grad=True), ref, "a valid call still works")

        ch, bl = np.ascontiguousarray(child, dtype=np.int32), np.ascontiguousarray(blen)
        ll, dt = np.empty(4), np.empty((4, 17))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        raw = lambda P, d, l, t: ctx._check(ctx._lib.phylo_trees_grad_model(ctx._h, C.c_int(4), p(ch), p(bl), C.c_int(P), d, None, l, None, t,
                                                                            None, None))
        refused(lambda: raw(0, p(dirs), p(ll), p(dt)), 'P=0')
        refused(lambda: raw(17, p(np.zeros((17, 4, 4))), p(ll), p(dt)), 'P=17')
        refused(lambda: ctx.trees_grad_model(child, blen, np.zeros((17, 4, 4))), 'P=17')
        refused(lambda: raw(16, None, p(ll), p(dt)), 'NULL')
        refused(lambda: raw(16, p(dirs), None, p(dt)), 'NULL')
        refused(lambda: raw(16, p(dirs), p(ll), None), 'NULL')
        for v in (np.nan, np.inf):
            d = dirs.copy()
            d[3, 2, 1] = v
            refused(lambda: ctx.trees_grad_model(child, blen, d), 'direction 3, entry 9')
        c = child.copy(); c[2, 2] = [6, 0]
        refused(lambda: ctx.trees_grad_model(c, blen, dirs), 'tree 2, row 2')        # a leaf used twice
        b = blen.copy(); b[2, 1, 1] = -1e-9
        refused(lambda: ctx.trees_grad_model(child, b, dirs), 'tree 2, row 1')       # a negative length
        with pytest.raises(ValueError):
            ctx.trees_grad_model(child, blen, np.zeros((3, 4, 3)))
        with pytest.raises(ValueError):
            ctx.trees_grad_model(child[:, :3], blen[:, :3], dirs)


# ---- 7. what the call leaves alone ------------------------------------------------------------------------------------------
def test_sweep_backward_summary_and_scratch_are_left_alone():
    g = load_dataset('primate_data')['genome'][:6, 100:170].copy()
    N, S, K, seed = 6, 70, 64, 5
    pi = np.array([[0.3, 0.2, 0.2, 0.3]])
    Q = model.get_Q(model.init_y_q())
    dirs = directions(12, Q)
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
        tg = ctx.trees_grad(child[:7], blen[:7], want_curv=True)
        tn = ctx.trees_nni(child[:7], blen[:7])
        mll, dth, mgrad, dpr = ctx.trees_grad_model(child, blen, dirs, want_grad=True)   # between a sweep and its pending reverse pass
        assert np.isfinite(dth).all() and np.isfinite(dpr).all() and np.isfinite(mgrad).all()
        np.testing.assert_array_equal(bits(mll[:7]), bits(ll))
        grad2 = ctx.sweep_backward()
        again = ctx.sweep_fetch()
        for key in ('log_weights', 'log_likelihood', 'left_branches', 'right_branches'):
            np.testing.assert_array_equal(bits(again[key]), bits(out[key]), err_msg=key)
        np.testing.assert_array_equal(again['ancestors'], out['ancestors'])
        assert bits(again['logZ']) == bits(out['logZ'])
        for key in ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q'):
            np.testing.assert_array_equal(bits(grad2[key]), bits(grad[key]), err_msg=key)
        # the scratch of sections 11 to 14: the same calls give the same bits afterwards
        l2, s2 = ctx.trees_loglik(child[:7], blen[:7], want_sites=True)
        np.testing.assert_array_equal(bits(s2), bits(sites))
        np.testing.assert_array_equal(bits(ctx.rell(sites, 50, 3, want_reps=True)['rep_loglik']), bits(rl['rep_loglik']))
        same(ctx.trees_grad(child[:7], blen[:7], want_curv=True), tg, "trees_grad before and after")
        same(ctx.trees_nni(child[:7], blen[:7]), tn, "trees_nni before and after")
        # a tree summary made before the call still has its branch pass
        tab = ctx.tree_summary()
        ctx.trees_grad_model(child[:3], blen[:3], dirs)
        tb = ctx.tree_branches(tab)
        assert np.isfinite(tb['leaf_stats']).all()
        third = ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)   # the next sweep's bits
        np.testing.assert_array_equal(bits(third['log_weights']), bits(out['log_weights']))
