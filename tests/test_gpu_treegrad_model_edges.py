"""phylo_trees_grad_model on the device where test_gpu_treegrad_model.py stops (inputs:
treegrad_edges_cases.py and trees_edges_cases.py).  B: 129 to 512 taxa in every shape, generic leaves and three tiles at 512,
16 directions on the deepest recursion.  C: 131 trees of 512 taxa in one chunk under one direction, so that three workgroups of
ptm_updown take a second item and reuse their node store and their LDS sums.  D: site factors near the floor of the double
range, at every place of trees_edges_cases.PLACES: below 2^-1020 every derivative of the tree is NaN beside
phylo_trees_loglik's loglik bits; at and above it they are those of the unscaled alignment.

ptm_updown and ptm_dirmats are kernels of their own; what test_gpu_trees_edges.py shows of ptg_updown says nothing about them.
Every precondition is asserted from the NumPy restatement (fed with the device's branch matrices) before anything is compared."""
import functools

import numpy as np
import pytest

import treegrad_edges_cases as GC
import treegrad_ref as TR
import trees_edges_cases as EC
from test_gpu_treegrad_model import close, reference, same
from test_gpu_trees_edges import compute_units, device_matrices
from test_gpu_trees_loglik import bits, make_ctx
from treegrad_edges_cases import TOL_MODEL_BIG
from trees_edges_cases import FLOOR, PRIOR, ROOMY

pytestmark = pytest.mark.gpu


def full_call(ctx, child, blen, dirs):
    return ctx.trees_grad_model(child, blen, dirs, prior=PRIOR, want_grad=True)


def bit_identities(ctx, child, blen, dirs, full, per_chunk, what):
    """loglik against phylo_trees_loglik, grad against phylo_trees_grad; the calls without grad, without dprior and on the
    reversed set: the bits of the full call (ll, dtheta, grad, dprior)"""
    ll, dth, grad, dpr = full
    np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)), err_msg=what + ": loglik against phylo_trees_loglik")
    np.testing.assert_array_equal(bits(grad), bits(ctx.trees_grad(child, blen, prior=PRIOR)[1]), err_msg=what + ": grad against phylo_trees_grad")
    same(ctx.trees_grad_model(child, blen, dirs, prior=PRIOR), (ll, dth, dpr), what + ": without grad")
    assert ctx.last_trees_stats['n_launches'] % (per_chunk - 2) == 0
    same(ctx.trees_grad_model(child, blen, dirs, prior=PRIOR, want_grad=True, want_prior=False), (ll, dth, grad), what + ": without dprior")
    rev = full_call(ctx, child[::-1], blen[::-1], dirs)
    same([a[::-1] for a in rev], full, what + ": the set reversed")


# ---- B. 129 to 512 taxa ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.BIG))
def test_many_taxa(name, monkeypatch):
    kw = EC.BIG[name]
    N, S, tile = kw['N'], kw['S'], kw.get('tile')
    g, child, blen, Q = EC.big_case(name)
    n = child.shape[0]
    P = 16 if name in ('caterpillar-N512', 'generic-balanced-N512') else 4
    dirs = GC.model_directions(P, Q)
    per_chunk = 7 if kw.get('generic') else 8                             # coded leaves: the gap rows of M too
    sample = [0, 2]
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR, tile=tile) as ctx:
        L = TR.trees_site_factors(child[sample], device_matrices(ctx, blen[sample]), PRIOR, g)
        assert (L >= ROOMY).all() and np.isfinite(L).all()                # the precondition, before anything is compared
        assert -(-S // ctx.site_tile()) == (3 if tile else 1)
        full = full_call(ctx, child, blen, dirs)
        st = ctx.last_trees_stats
        assert st['units'] == n * S * (N - 1) * (1 + P) and st['n_launches'] == per_chunk
        assert np.isfinite(full[0]).all()
        rll, rdth, rdpr, sc_t, sc_p = reference(ctx, child[sample], blen[sample], Q, dirs, PRIOR, g, tile=ctx.site_tile())
        np.testing.assert_allclose(full[0][sample], rll, rtol=1e-12, atol=0)
        close("%s P%d dtheta" % (name, P), full[1][sample], rdth, sc_t, TOL_MODEL_BIG)
        close("%s P%d dprior" % (name, P), full[3][sample], rdpr, sc_p, TOL_MODEL_BIG)
        bit_identities(ctx, child, blen, dirs, full, per_chunk, name)
    monkeypatch.setenv('PHYLO_TREES_CHUNK', '2')                          # read when the context is created
    with make_ctx(g, Q, pi=PRIOR, tile=tile) as ctx:
        same(full_call(ctx, child, blen, dirs), full, "chunks of 2")
        assert ctx.last_trees_stats['n_launches'] == 3 * per_chunk


# ---- C. a workgroup's second 512-taxon item ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ['same', 'mixed'])
def test_strided_items_512_taxa(which, monkeypatch):
    """P = 1: a tree takes 466 128 B of the 64 MiB chunk (ptm_make_plan), so all 131 trees ride in one chunk; the node store caps
    the grid at 256 MiB / (511 2 2 KiB) = 128 workgroups, and workgroups 0 to 2 take trees 128 to 130 as their second items"""
    g, child, blen, Q = EC.large_strided(which == 'mixed')
    T = child.shape[0]
    dirs = GC.model_directions(1, Q)
    sample = [0, 1, 127, 128, 129, 130]
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        assert -(-g.shape[1] // ctx.site_tile()) == 1 and T == 131
        full = full_call(ctx, child, blen, dirs)
        assert ctx.last_trees_stats['n_launches'] == 8                    # one chunk: items > grid, workgroups stride
        assert EC.updown_cap(512, compute_units()) == 128
        if which == 'mixed':
            for w in range(128, T):
                assert child[w].tobytes() != child[w - 128].tobytes()     # a second item of another row order
        L = TR.trees_site_factors(child[sample], device_matrices(ctx, blen[sample]), PRIOR, g)
        assert (L >= ROOMY).all() and np.isfinite(L).all()
        np.testing.assert_array_equal(bits(full[0]), bits(ctx.trees_loglik(child, blen, prior=PRIOR)), err_msg="loglik against phylo_trees_loglik")
        np.testing.assert_array_equal(bits(full[2]), bits(ctx.trees_grad(child, blen, prior=PRIOR)[1]), err_msg="grad against phylo_trees_grad")
        rll, rdth, rdpr, sc_t, sc_p = reference(ctx, child[sample], blen[sample], Q, dirs, PRIOR, g, tile=ctx.site_tile())
        np.testing.assert_allclose(full[0][sample], rll, rtol=1e-12, atol=0)
        close("N512 %s strided dtheta" % which, full[1][sample], rdth, sc_t, TOL_MODEL_BIG)
        close("N512 %s strided dprior" % which, full[3][sample], rdpr, sc_p, TOL_MODEL_BIG)
    monkeypatch.setenv('PHYLO_TREES_CHUNK', '128')
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        parts = full_call(ctx, child, blen, dirs)
        assert ctx.last_trees_stats['n_launches'] == 2 * 8
    same(full, parts, "strided against one item per workgroup")


# ---- D. the floor of the range ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unscaled():
    g, child, blen, Q = EC.scaled_base()
    dirs = GC.model_directions(12, Q)
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        assert ctx.site_tile() == 64
        got = full_call(ctx, child, blen, dirs)
        M = device_matrices(ctx, blen)
        _, _, _, sc_g, L0 = TR.trees_grad(child, M, Q, PRIOR, g, want_sites=True)
        ref = reference(ctx, child, blen, Q, dirs, PRIOR, g, tile=64)
    assert np.isfinite(got[0]).all() and (L0 > 2.0 ** -200).all()
    close("unscaled dtheta", got[1], ref[1], ref[3])
    close("unscaled dprior", got[3], ref[2], ref[4])
    for a in got + ref + (sc_g, L0):
        a.setflags(write=False)
    return g, child, blen, Q, dirs, got, ref, sc_g, L0


@pytest.mark.parametrize("place", EC.PLACES)
def test_scaled_sites(place):
    g, child, blen, Q, dirs, (ll0, dth0, grad0, dpr0), (_, _, _, sc_t0, sc_p0), sc_g0, L0 = unscaled()
    e = EC.scaled_exponents(place, L0)
    gs = EC.scaled_leaves(g, e)
    at = list(EC.SCALED_SITES)
    with make_ctx(gs, Q, pi=PRIOR, tile=64) as ctx:
        L = TR.trees_site_factors(child, device_matrices(ctx, blen), PRIOR, gs)
        print(place, "reference: scaled site factors in [%.3g, %.3g]" % (L[:, at].min(), L[:, at].max()))
        np.testing.assert_array_equal(np.delete(L, at, axis=1), np.delete(L0, at, axis=1))
        rll, rdth, rdpr, _, _ = reference(ctx, child, blen, Q, dirs, PRIOR, gs, tile=64)
        plain = ctx.trees_loglik(child, blen, prior=PRIOR)
        ll, dth, grad, dpr = full_call(ctx, child, blen, dirs)
        lean = ctx.trees_grad_model(child, blen, dirs, prior=PRIOR, want_prior=False)
        np.testing.assert_array_equal(bits(ll), bits(plain), err_msg="loglik against phylo_trees_loglik")
        np.testing.assert_array_equal(bits(lean[0]), bits(plain))
        np.testing.assert_array_equal(bits(grad), bits(ctx.trees_grad(child, blen, prior=PRIOR)[1]), err_msg="grad against phylo_trees_grad")
        shift = e.sum() * np.log(2.0)
        if place == '2^-900':
            assert (L[:, at] < 2.0 ** -880).all() and (L[:, at] > 2.0 ** -960).all()
            same((dth, grad, dpr, lean[1]), (dth0, grad0, dpr0, dth0), "2^-900: the unscaled call's bits")
            np.testing.assert_allclose(ll, ll0 - shift, rtol=1e-12, atol=0)
        elif place in EC.IN_RANGE:
            assert (L[:, at] >= FLOOR).all() and (L[:, at] <= ROOMY).all()
            if place == 'at-the-floor':
                assert (L[:, at].min(axis=0) < 2.0 ** -1019).all()
            assert np.isfinite(ll).all()
            np.testing.assert_allclose(ll, ll0 - shift, rtol=1e-12, atol=0)
            close(place + " dtheta against the restatement on the scaled alignment", dth, rdth, sc_t0)
            close(place + " dprior against the restatement on the scaled alignment", dpr, rdpr, sc_p0)
            close(place + " dtheta against the unscaled call", dth, dth0, sc_t0)
            close(place + " dprior against the unscaled call", dpr, dpr0, sc_p0)
            close(place + " grad against the unscaled call", grad, grad0, sc_g0)
            close(place + " dtheta alone against the unscaled call", lean[1], dth0, sc_t0)
        else:
            assert (L[:, at] < FLOOR).all() and np.isnan(rdth).all() and np.isnan(rdpr).all()
            if place == 'just-below':
                assert (L[:, at].max(axis=0) >= 2.0 ** -1021).all()
            if place == 'zero':
                assert (L[:, at] == 0).all() and (ll == -np.inf).all()
            else:
                assert (L[:, at] > 0).all() and np.isfinite(ll).all()
            assert np.isnan(dth).all() and np.isnan(grad).all() and np.isnan(dpr).all() and np.isnan(lean[1]).all()


def test_one_site_below_the_floor_spoils_its_tree_alone():
    """a set in which only SOME trees see a factor below the floor: the others keep what they have without it"""
    g, child, blen, Q, dirs, (ll0, dth0, grad0, dpr0), (_, rdth0, rdpr0, sc_t0, sc_p0), sc_g0, L0 = unscaled()
    gs = GC.scale_one_site(g, GC.one_site_below(L0))
    with make_ctx(gs, Q, pi=PRIOR, tile=64) as ctx:
        L = TR.trees_site_factors(child, device_matrices(ctx, blen), PRIOR, gs)
        out = (L < FLOOR).any(axis=1)
        assert 1 <= out.sum() < out.size and (L > 0).all(), L[:, 129]
        _, rdth, rdpr, _, _ = reference(ctx, child, blen, Q, dirs, PRIOR, gs, tile=64)
        assert np.isnan(rdth[out]).all() and np.isnan(rdpr[out]).all()    # the restatement first
        close("restatement, in-range trees, dtheta", rdth[~out], rdth0[~out], sc_t0[~out])
        close("restatement, in-range trees, dprior", rdpr[~out], rdpr0[~out], sc_p0[~out])
        ll, dth, grad, dpr = full_call(ctx, child, blen, dirs)
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)))
        assert np.isfinite(ll).all()
        assert np.isnan(dth[out]).all() and np.isnan(grad[out]).all() and np.isnan(dpr[out]).all()
        close("in-range trees, dtheta", dth[~out], dth0[~out], sc_t0[~out])
        close("in-range trees, dprior", dpr[~out], dpr0[~out], sc_p0[~out])
        close("in-range trees, grad", grad[~out], grad0[~out], sc_g0[~out])
