"""phylo_trees_nni on the device: the change of the log-likelihood of every tree of a set under each of
its nearest-neighbour interchanges.  loglik is held to phylo_trees_loglik's bits; delta to the NumPy restatement
(treenni_ref.py, fed with the device's own branch matrices) within TOL_NNI (S + sum_s |d_s| + |value|), and for N <= 12 loglik +
delta to phylo_trees_loglik of the explicitly built neighbour (apply_nni) within TOL_EXPL (S + sum_s |log L_s| + sum_s
|log L'_s|) -- both bounds set from 50-digit arithmetic before the kernel ran (treenni_cases.py).  Then: repeated, chunked and
strided calls bit for bit, the NaN rules, refusals, what the call leaves alone.

Every test here needs Context.trees_nni: AttributeError without it."""
import ctypes as C

import numpy as np
import pytest

import treegrad_ref as TR
import treenni_cases as NC
import treenni_ref as NR
import trees_edges_cases as EC
from oracle import cpu_ref as O
from phylo_amd import _ffi, model
from phylo_amd import treepost as TP
from phylo_amd.datasets import load_dataset
from phylo_amd.treesearch import apply_nni, nni_moves
from test_gpu_trees_edges import compute_units
from test_gpu_trees_loglik import PI, alignment, bits, gtr_Q, make_ctx, random_trees, shaped_trees
from treenni_cases import PRIOR, TOL_EXPL, TOL_NNI
from trees_cases import balanced_rows, caterpillar_rows

pytestmark = pytest.mark.gpu
T = 37


def device_matrices(ctx, blen):
    return ctx.expm_batched(np.asarray(blen).reshape(-1)).reshape(np.shape(blen) + (4, 4))


def reference(ctx, child, blen, prior, g):
    """the restatement on the device's own matrices: expm differences stay out of the comparison"""
    return NR.trees_nni(child, device_matrices(ctx, blen), prior, g)


def close(name, got, ref, absd, S, tol=TOL_NNI):
    """NaN where the restatement has NaN, -inf where it has -inf, elsewhere within TOL_NNI (S + sum |d_s| + |value|) (tol: the
    bound of the deep trees, treenni_cases.TOL_NNI_BIG).  Returns the worst ratio to the bound."""
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=name + ": NaN entries")
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref), err_msg=name + ": -inf entries")
    at = np.isfinite(ref)
    assert np.isfinite(got[at]).all(), name
    err = np.abs(got[at] - ref[at]) / (S + absd[at] + np.abs(ref[at]))
    print("%s: worst |device - restatement| / (S + sum |d_s| + |value|) = %.3g (bound %.3g) over %d entries, %d -inf, %d NaN"
          % (name, err.max() if err.size else 0.0, tol, err.size, np.isneginf(ref).sum(), np.isnan(ref).sum()))
    assert (err <= tol).all(), (name, float(err.max()), tol)
    return float(err.max()) / tol if err.size else 0.0


def missing_moves(child):
    """[T][N-1][2] bool: the entries whose move does not exist"""
    out = np.ones(child.shape, dtype=bool)
    for t, c in enumerate(child):
        for mv in nni_moves(c):
            out[t][mv] = False
    return out


def explicit(name, ctx, child, blen, ll, delta, prior, S, tol=TOL_EXPL, moves=nni_moves):
    """loglik + delta against phylo_trees_loglik of every explicitly built neighbour (moves: which of a tree's moves; tol: the
    bound of the deep trees, treenni_cases.TOL_EXPL_BIG).  Returns the worst ratio to the bound."""
    _, sites = ctx.trees_loglik(child, blen, prior=prior, want_sites=True)
    with np.errstate(divide='ignore'):
        a0 = np.abs(np.log(sites)).sum(axis=1)
    cs, bs, at = [], [], []
    for t in range(child.shape[0]):
        for mv in moves(child[t]):
            c2, b2 = apply_nni(child[t], blen[t], *mv)
            cs.append(c2)
            bs.append(b2)
            at.append((t,) + mv)
    if not cs:
        return 0.0
    ll2, sites2 = ctx.trees_loglik(np.array(cs), np.array(bs), prior=prior, want_sites=True)
    worst = 0.0
    for (t, r, sd), x, s2 in zip(at, ll2, sites2):
        lhs = ll[t] + delta[t, r, sd]
        if np.isneginf(x) or np.isneginf(lhs):
            assert x == lhs, (name, t, r, sd, lhs, x)
            continue
        err = abs(lhs - x) / (S + a0[t] + np.abs(np.log(s2)).sum())
        worst = max(worst, err)
        assert err <= tol, (name, t, r, sd, lhs, x, err, tol)
    print("%s: worst |(loglik + delta) - loglik of the neighbour| / (S + sum |log L| + sum |log L'|) = %.3g (bound %.3g) over %d moves"
          % (name, worst, tol, len(at)))
    return worst / tol


# ---- 1. shapes and conditions ------------------------------------------------------------------------------------------------
def case(N, S, **kw):
    return dict(N=N, S=S, **kw)


CASES = {
    'N5-S1': case(5, 1), 'N5-S63': case(5, 63), 'N12-S65': case(12, 65), 'N12-S129': case(12, 129), 'N12-S300': case(12, 300),
    'N5-caterpillar': case(5, 65, shape=caterpillar_rows), 'N5-balanced': case(5, 65, shape=balanced_rows),
    'N12-caterpillar': case(12, 130, shape=caterpillar_rows), 'N12-balanced': case(12, 130, shape=balanced_rows, gaps=True),
    'N64-random': case(64, 65, n=5), 'N64-caterpillar': case(64, 65, shape=caterpillar_rows, n=5),
    'N64-balanced': case(64, 65, shape=balanced_rows, n=5, gaps=True), 'N128-balanced': case(128, 65, shape=balanced_rows, n=3),
    'two-tiles': case(12, 100, tile=64), 'three-tiles': case(12, 130, tile=64, gaps=True),
    'generic': case(12, 130, generic=True), 'generic-gaps-three-tiles': case(5, 130, generic=True, gaps=True, tile=64),
    'gaps': case(12, 130, gaps=True), 'jc69': case(12, 130, jc=True), 'jc69-gaps-N5': case(5, 129, jc=True, gaps=True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_reference(name, monkeypatch):
    kw = CASES[name]
    N, S, jc, n = kw['N'], kw['S'], kw.get('jc', False), kw.get('n', T)
    g = alignment(N, S, 100 + N + S, kw.get('gaps', False), kw.get('generic', False))
    Q = O.jc_Q() if jc else gtr_Q()
    child, blen = shaped_trees(kw['shape'], N, 5, n) if 'shape' in kw else random_trees(N, 5, n)
    assert (blen == 0).any()                                              # trees with zero-length branches
    chunk = 2 if n < T else 5
    monkeypatch.setenv('PHYLO_TREES_CHUNK', str(chunk))                   # read when the context is created: several chunks
    with make_ctx(g, Q, jc=jc, tile=kw.get('tile')) as ctx:
        ll, delta = ctx.trees_nni(child, blen, prior=PRIOR)
        st = ctx.last_trees_stats
        assert st['units'] == n * S * (N - 1) and st['sweep_ms'] > 0
        assert st['n_launches'] == -(-n // chunk) * (4 if kw.get('generic') else 5)     # coded leaves: the gap rows too
        assert delta.shape == blen.shape
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)), err_msg="loglik against phylo_trees_loglik")
        assert np.isfinite(ll).all()
        np.testing.assert_array_equal(np.isnan(delta), missing_moves(child), err_msg="NaN exactly where a move does not exist")
        rll, rdelta, absd = reference(ctx, child, blen, PRIOR, g)
        np.testing.assert_allclose(ll, rll, rtol=1e-12, atol=0)
        close(name, delta, rdelta, absd, S)
        ll2, delta2 = ctx.trees_nni(child, blen, prior=PRIOR)              # a repeat call: the same bits
        np.testing.assert_array_equal(bits(ll2), bits(ll))
        np.testing.assert_array_equal(bits(delta2), bits(delta))
        rev = ctx.trees_nni(child[::-1], blen[::-1], prior=PRIOR)          # a tree's bits do not depend on its place
        np.testing.assert_array_equal(bits(rev[0][::-1]), bits(ll))
        np.testing.assert_array_equal(bits(rev[1][::-1]), bits(delta))
        if N <= 12:
            explicit(name, ctx, child[:8], blen[:8], ll, delta, PRIOR, S)


def test_two_taxa_have_no_move():
    g = alignment(2, 130, 5)
    child, blen = random_trees(2, 5, 3)
    with make_ctx(g, gtr_Q()) as ctx:
        ll, delta = ctx.trees_nni(child, blen, prior=PRIOR)
        assert delta.shape == (3, 1, 2) and np.isnan(delta).all()
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)))


@pytest.mark.parametrize("N", [3, 4])
@pytest.mark.parametrize("generic", [False, True])
def test_every_rooted_shape(N, generic):
    """N = 3 and 4: every rooted shape, a root with a leaf child on either side included, under several labellings"""
    S = 65
    rng = np.random.default_rng(N)
    g = alignment(N, S, 7 + N, gaps=True, generic=generic)
    child, blen = [], []
    for c in NC.rooted_shapes(N):
        for _ in range(3):
            perm = rng.permutation(N)
            child.append(np.where(c < N, perm[np.minimum(c, N - 1)], c).astype(np.int32))
            blen.append(rng.exponential(0.1, (N - 1, 2)))
    child, blen = np.array(child), np.array(blen)
    with make_ctx(g, gtr_Q()) as ctx:
        ll, delta = ctx.trees_nni(child, blen, prior=PRIOR)
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)))
        miss = missing_moves(child)
        assert miss[:, :-1].sum() == 0 and miss[:, -1].any() and (N == 3 or not miss[:, -1].all())
        np.testing.assert_array_equal(np.isnan(delta), miss)
        rll, rdelta, absd = reference(ctx, child, blen, PRIOR, g)
        close("N%d shapes" % N, delta, rdelta, absd, S)
        explicit("N%d shapes" % N, ctx, child, blen, ll, delta, PRIOR, S)


def test_prior_none_is_the_models_pi():
    g = alignment(7, 70, 3, gaps=True)
    pi = np.array([0.4, 0.3, 0.2, 0.1])
    child, blen = random_trees(7, 9, 5)
    with make_ctx(g, gtr_Q(), pi=pi) as ctx:
        a, b = ctx.trees_nni(child, blen), ctx.trees_nni(child, blen, prior=pi)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(bits(x), bits(y))
        assert not np.array_equal(bits(a[1]), bits(ctx.trees_nni(child, blen, prior=PI)[1]))


def test_impossible_neighbours_are_minus_infinity():
    """v = (0, 1) with leaf 1 on a zero-length branch, its sibling leaf 2 on a zero-length branch: the move that joins 1 and 2
    gives every site at which they differ the likelihood 0; the tree itself is fine"""
    N, S = 4, 65
    g = alignment(N, S, 19)
    assert (g[1] != g[2]).any()
    child = np.array([[[0, 1], [4, 2], [5, 3]]] * 2, dtype=np.int32)
    blen = np.array([[[0.1, 0.0], [0.1, 0.0], [0.2, 0.3]], [[0.1, 0.05], [0.1, 0.02], [0.2, 0.3]]])
    with make_ctx(g, gtr_Q()) as ctx:
        ll, delta = ctx.trees_nni(child, blen, prior=PRIOR)
        rll, rdelta, absd = reference(ctx, child, blen, PRIOR, g)
        assert np.isfinite(ll).all() and rdelta[0, 0, 0] == -np.inf and np.isneginf(rdelta).sum() == 1
        close("zero lengths", delta, rdelta, absd, S)
        explicit("zero lengths", ctx, child, blen, ll, delta, PRIOR, S)


# ---- 2. the same bits in chunks, and with more items than workgroups ----------------------------------------------------------
def test_chunks_give_the_same_bits(monkeypatch):
    g = alignment(12, 130, 31, gaps=True)
    child, blen = random_trees(12, 6)
    got = {}
    for chunk in ('0', '5', '1'):
        monkeypatch.setenv('PHYLO_TREES_CHUNK', chunk)
        with make_ctx(g, gtr_Q(), tile=64) as ctx:
            got[chunk] = ctx.trees_nni(child, blen)
            assert ctx.last_trees_stats['n_launches'] == 5 * {'0': 1, '5': 8, '1': 37}[chunk]
    for chunk in ('5', '1'):
        for a, b in zip(got[chunk], got['0']):
            np.testing.assert_array_equal(bits(a), bits(b))


@pytest.mark.parametrize("generic", [False, True], ids=['coded', 'generic'])
def test_more_items_than_workgroups(generic, monkeypatch):
    """N = 5, three tiles, 8 CUs + 5 items or more in ONE chunk (a workgroup takes a second item) against the same trees in chunks
    of one item per workgroup, bit for bit; and against the restatement on the trees of the second items"""
    cus = compute_units()
    cap = EC.updown_cap(5, cus)
    n = EC.strided_T(5, 3, cus)
    g, child, blen, Q = EC.small_strided(n, generic=generic)
    S = g.shape[1]
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        assert -(-S // ctx.site_tile()) == 3 and 3 * n >= cap + 5 and (3 * n) % cap != 0
        full = ctx.trees_nni(child, blen, prior=PRIOR)
        assert ctx.last_trees_stats['n_launches'] == (4 if generic else 5)       # one chunk
        np.testing.assert_array_equal(bits(full[0]), bits(ctx.trees_loglik(child, blen, prior=PRIOR)))
        sample = sorted(set(range(8)) | set(range(cap // 3 - 2, n)))
        _, rdelta, absd = reference(ctx, child[sample], blen[sample], PRIOR, g)
        close("strided", full[1][sample], rdelta, absd, S)
    chunk = cap // 3
    monkeypatch.setenv('PHYLO_TREES_CHUNK', str(chunk))
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        parts = ctx.trees_nni(child, blen, prior=PRIOR)
        assert ctx.last_trees_stats['n_launches'] == -(-n // chunk) * (4 if generic else 5)
    for a, b in zip(full, parts):
        np.testing.assert_array_equal(bits(a), bits(b))


# ---- 3. the NaN rules ----------------------------------------------------------------------------------------------------------
def test_a_dead_site_gives_nan():
    N, S = 5, 70
    g = alignment(N, S, 22, generic=True)
    g[2, 66] = 0.0                                                       # a generic leaf row of zeros kills the site in every tree
    child, blen = random_trees(N, 4, 3)
    with make_ctx(g, gtr_Q()) as ctx:
        ll, delta = ctx.trees_nni(child, blen, prior=PI)
        assert (ll == -np.inf).all() and np.isnan(delta).all()
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PI)))


def test_one_site_below_the_floor_spoils_its_tree_alone():
    """trees_edges_cases' construction: one site's factor scaled through two generic leaves so that SOME trees see it below 2^-1020;
    those get NaN in every entry beside an unchanged finite loglik, the others stay within the tolerance of the unscaled call"""
    g, child, blen, Q = EC.scaled_base()
    S = g.shape[1]
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        L0 = TR.trees_site_factors(child, device_matrices(ctx, blen), PRIOR, g)
        _, want = ctx.trees_nni(child, blen, prior=PRIOR)
        _, rdelta, absd = reference(ctx, child, blen, PRIOR, g)
        close("unscaled", want, rdelta, absd, S)
    s = 129
    order = np.argsort(L0[:, s])
    e = int(np.frexp(L0[order[2], s])[1]) + 1020                          # the third smallest lands in [2^-1021, 2^-1020) ...
    gs = g.copy()
    gs[0, s], gs[1, s] = np.ldexp(g[0, s], -(e // 2)), np.ldexp(g[1, s], -(e - e // 2))
    with make_ctx(gs, Q, pi=PRIOR, tile=64) as ctx:
        L = TR.trees_site_factors(child, device_matrices(ctx, blen), PRIOR, gs)
        out = (L < TR.FLOOR).any(axis=1)
        assert 1 <= out.sum() < out.size and (L > 0).all(), L[:, s]
        ll, delta = ctx.trees_nni(child, blen, prior=PRIOR)
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)))
        assert np.isfinite(ll).all() and np.isnan(delta[out]).all()
        rdelta2 = reference(ctx, child, blen, PRIOR, gs)[1]
        assert np.isnan(rdelta2[out]).all()
        # the in-range trees keep every entry (no tolerance is claimed for them here: beside a site factor just above 2^-1020 a
        # neighbour's own factor may be subnormal, where neither the device nor the restatement holds 53 bits)
        np.testing.assert_array_equal(np.isnan(delta[~out]), missing_moves(child[~out]))
        np.testing.assert_allclose(delta[~out], want[~out], rtol=1e-6, atol=1e-6)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing():
    N, S = 5, 70
    g = alignment(N, S, 41)
    child, blen = random_trees(N, 8, 4)
    child[2] = np.array([[0, 1], [2, 3], [6, 4], [5, 7]], dtype=np.int32)
    with _ffi.Context(4, N, S) as ctx:
        with pytest.raises(_ffi.PhyloError) as e:
            ctx.trees_nni(child, blen)
        assert e.value.code == -6                                          # PHYLO_ESTATE: no leaves, no model
        ctx.set_leaves(g)
        with pytest.raises(_ffi.PhyloError) as e:
            ctx.trees_nni(child, blen)
        assert e.value.code == -6                                          # no model
        ctx.set_model(gtr_Q(), PI, np.full(N - 1, 10.0), np.full(N - 1, 10.0))
        ref = ctx.trees_nni(child, blen)

        def refused(call, what):
            with pytest.raises(_ffi.PhyloError) as e:
                call()
            assert e.value.code == -1 and what in str(e.value), str(e.value)
            for a, b in zip(ctx.trees_nni(child, blen), ref):               # a valid call still works
                np.testing.assert_array_equal(bits(a), bits(b))

        c = child.copy(); c[2, 2] = [6, 0]
        refused(lambda: ctx.trees_nni(c, blen), 'tree 2, row 2')             # a leaf used twice
        c2 = child.copy(); c2[2, 3] = [5, -1]
        refused(lambda: ctx.trees_nni(c2, blen), 'tree 2, row 3')            # no child at all
        c3 = child.copy(); c3[1, 0] = [0, 6]
        refused(lambda: ctx.trees_nni(c3, blen), 'tree 1, row 0')            # a child from a later row
        for v in (np.nan, -1e-9, np.inf):
            b = blen.copy(); b[2, 1, 1] = v
            refused(lambda: ctx.trees_nni(child, b), 'tree 2, row 1')        # a negative (or non-finite) length
        ch, bl = np.ascontiguousarray(child, dtype=np.int32), np.ascontiguousarray(blen)
        ll, dl = np.empty(4), np.empty(blen.shape)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        raw = lambda n, *a: ctx._check(ctx._lib.phylo_trees_nni(ctx._h, C.c_int(n), *a))
        refused(lambda: raw(4, p(ch), p(bl), None, None, p(dl), None), 'NULL')      # NULL outputs and inputs
        refused(lambda: raw(4, p(ch), p(bl), None, p(ll), None, None), 'NULL')
        refused(lambda: raw(4, None, p(bl), None, p(ll), p(dl), None), 'NULL')
        refused(lambda: raw(4, p(ch), None, None, p(ll), p(dl), None), 'NULL')
        refused(lambda: raw(0, p(ch), p(bl), None, p(ll), p(dl), None), 'T >= 1')
        refused(lambda: raw(-3, p(ch), p(bl), None, p(ll), p(dl), None), 'T >= 1')
        raw(4, p(ch), p(bl), None, p(ll), p(dl), None)                       # perf may be NULL
        np.testing.assert_array_equal(bits(dl), bits(ref[1]))
        with pytest.raises(ValueError):
            ctx.trees_nni(child[:, :3], blen[:, :3])


# ---- 5. what the call leaves alone ---------------------------------------------------------------------------------------------
def test_sweep_gradients_and_scores_are_left_alone():
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
        tg = ctx.trees_grad(child[:7], blen[:7], want_curv=True)
        nll, delta = ctx.trees_nni(child, blen)                             # between a sweep and its pending reverse pass
        np.testing.assert_array_equal(np.isnan(delta), missing_moves(child))
        np.testing.assert_array_equal(bits(nll[:7]), bits(ll))
        grad2 = ctx.sweep_backward()
        again = ctx.sweep_fetch()
        for key in ('log_weights', 'log_likelihood', 'left_branches', 'right_branches'):
            np.testing.assert_array_equal(bits(again[key]), bits(out[key]), err_msg=key)
        np.testing.assert_array_equal(again['ancestors'], out['ancestors'])
        assert bits(again['logZ']) == bits(out['logZ'])
        for key in ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q'):
            np.testing.assert_array_equal(bits(grad2[key]), bits(grad[key]), err_msg=key)
        l2, s2 = ctx.trees_loglik(child[:7], blen[:7], want_sites=True)      # the scratch of sections 11 and 13
        np.testing.assert_array_equal(bits(s2), bits(sites))
        for a, b in zip(ctx.trees_grad(child[:7], blen[:7], want_curv=True), tg):
            np.testing.assert_array_equal(bits(a), bits(b))
        third = ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)   # the next sweep's bits
        np.testing.assert_array_equal(bits(third['log_weights']), bits(out['log_weights']))
