"""Scored tree sets on the device where the other suites stop (DESIGN.md sections 11, 11b, 13; inputs: trees_edges_cases.py).
A: 129 to 512 taxa -- schedules of 8 and 9 slots, both site-step counts of pt2_unroll -- through phylo_trees_loglik, its site
factors, phylo_trees_loglik_rates and phylo_trees_grad.  B: more work items than ptg_updown has workgroups, so that a workgroup
reuses its node store and its LDS sums for a second item, against the same trees in chunks that fit under the cap.  C: site
factors near the floor of the double range: below 2^-1020 every derivative of the tree is NaN beside the loglik bits of
phylo_trees_loglik; at and above it the derivatives are those of the unscaled alignment.

Every precondition is asserted from the NumPy restatement (fed with the device's branch matrices) before anything is compared."""
import functools
import subprocess
import sys

import mpmath as mp
import numpy as np
import pytest

import rates_ref
import site_product_ref as SP
import treegrad_ref as TR
import trees_edges_cases as EC
from oracle import c_oracle as CO
from oracle import cpu_ref as O
from phylo_amd import _ffi
from phylo_amd import rates as R
from phylo_amd.treeopt import OutOfRangeError, optimize_branches
from test_gpu_treegrad import close, reference
from test_gpu_trees_loglik import bits, make_ctx, one_by_one
from trees_cases import rows_to_nodes
from trees_edges_cases import FLOOR, PRIOR, ROOMY

pytestmark = pytest.mark.gpu


def device_matrices(ctx, blen):
    return ctx.expm_batched(np.asarray(blen).reshape(-1)).reshape(np.shape(blen) + (4, 4))


def same_bits(got, want, what):
    for name, a, b in zip(('loglik', 'grad', 'curv', 'extra'), got, want):
        np.testing.assert_array_equal(bits(a), bits(b), err_msg="%s: %s" % (what, name))


# ---- A. 129 to 512 taxa --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.BIG))
def test_many_taxa(name, monkeypatch):
    kw = EC.BIG[name]
    N, S, tile = kw['N'], kw['S'], kw.get('tile')
    g, child, blen, Q = EC.big_case(name)
    n = child.shape[0]
    rates, weights = R.rate_model(0.5, 4, 0.2)                            # four discrete Gamma categories and an invariant class
    depths = [_ffi.debug_tree_schedule(c, b)[1] for c, b in zip(child, blen)]
    assert depths == [EC.su_depth(c) for c in child]
    if kw['shape'] == 'balanced':                                         # floor(log2 N) slots, the most N taxa can need (section 11)
        assert depths[0] == {129: 7, 257: 8, 512: 9}[N]
    if kw['shape'] == 'caterpillar':
        assert depths[0] == 1 and max(depths) <= 2                        # four site steps per pass
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    CO.set_site_tile(tile or 0)                                           # the oracle takes the context's site tile
    try:
        with make_ctx(g, Q, pi=PRIOR, tile=tile) as ctx:
            ntiles = -(-S // ctx.site_tile())
            assert ntiles == (3 if tile else 1)
            rll, rgrad, rcurv, scale, L = TR.trees_grad(child, device_matrices(ctx, blen), Q, PRIOR, g, want_sites=True)
            print("%s: reference site factors in [%.3g, %.3g]" % (name, L.min(), L.max()))
            assert (L >= ROOMY).all() and np.isfinite(L).all()            # the precondition, before anything is compared
            # phylo_trees_loglik: the bits of phylo_tree_loglik and of the C oracle, tree by tree
            ll = ctx.trees_loglik(child, blen, prior=PRIOR)
            assert ctx.last_trees_stats['units'] == n * S * (N - 1)
            dev, ora, roots = one_by_one(ctx, g, Q, PRIOR, child, blen)
            assert np.isfinite(ll).all()
            np.testing.assert_array_equal(bits(ll), bits(dev), err_msg="against phylo_tree_loglik")
            np.testing.assert_array_equal(bits(ll), bits(ora), err_msg="against the C oracle")
            np.testing.assert_allclose(ll, rll, rtol=1e-12, atol=0)
            # the site factors multiply back to loglik
            ll_s, sites = ctx.trees_loglik(child, blen, prior=PRIOR, want_sites=True)
            np.testing.assert_array_equal(bits(ll_s), bits(ll))
            assert sites.shape == (n, S) and (sites > 0).all()
            np.testing.assert_allclose(sites, roots @ PRIOR, rtol=1e-14, atol=0)
            np.testing.assert_allclose(sites, L, rtol=1e-14, atol=0)
            for t in range(n):
                exact, bound = SP.row_bound(sites[t], ctx.site_tile())
                assert float(abs(mp.mpf(float(ll[t])) - exact)) <= bound, (t, ll[t])
            # phylo_trees_loglik_rates: composition, the mixing chain, the sum (what test_gpu_trees_rates.py holds it to)
            C = rates.size
            rl, rsites, cats = ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR, want_sites=True, want_cats=True)
            assert ctx.last_trees_stats['units'] == n * S * (N - 1) * C
            np.testing.assert_array_equal(bits(ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR)), bits(rl))
            for c in range(C):
                _, f = ctx.trees_loglik(child, rates[c] * blen, prior=PRIOR, want_sites=True)
                np.testing.assert_array_equal(bits(cats[:, c, :]), bits(f), err_msg="category %d" % c)
            mixed = np.array([rates_ref.mix(weights, cats[t]) for t in range(n)])
            np.testing.assert_array_equal(bits(rsites), bits(mixed), err_msg="the mixing chain")
            assert np.isfinite(rl).all() and (rsites > 0).all()
            for t in range(n):
                exact, bound = SP.row_bound(rsites[t], ctx.site_tile())
                assert float(abs(mp.mpf(float(rl[t])) - exact)) <= bound, (t, rl[t])
                left, right, bl, br = rows_to_nodes(child[t], blen[t])
                mix = np.zeros(S)
                with np.errstate(divide='ignore'):                            # (the invariant class has factors that are 0)
                    for c in range(C):
                        _, root = O.tree_loglik(Q, PRIOR, 2 * N - 1, left, right, rates[c] * bl, rates[c] * br, 2 * N - 2, g)
                        mix += weights[c] * (root @ PRIOR)
                assert rl[t] == pytest.approx(float(np.sum(np.log(mix))), rel=1e-12), t
            # phylo_trees_grad
            got = ctx.trees_grad(child, blen, prior=PRIOR, want_curv=True)
            assert ctx.last_trees_stats['n_launches'] == (5 if kw.get('generic') else 6)
            np.testing.assert_array_equal(bits(got[0]), bits(ll), err_msg="loglik against phylo_trees_loglik")
            close(name + " grad", got[1], rgrad, scale)
            close(name + " curv", got[2], rcurv, scale)
            same_bits(ctx.trees_grad(child, blen, prior=PRIOR), got[:2], "without curvature")
            rev = ctx.trees_grad(child[::-1], blen[::-1], prior=PRIOR, want_curv=True)
            same_bits([a[::-1] for a in rev], got, "the trees in reverse order")
        monkeypatch.setenv('PHYLO_TREES_CHUNK', '2')                      # read when the context is created
        with make_ctx(g, Q, pi=PRIOR, tile=tile) as ctx:
            same_bits(ctx.trees_loglik(child, blen, prior=PRIOR, want_sites=True), (ll, sites), "chunks of 2, plain")
            assert ctx.last_trees_stats['n_launches'] > 4
            same_bits(ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR, want_sites=True), (rl, rsites), "chunks of 2, rates")
            same_bits(ctx.trees_grad(child, blen, prior=PRIOR, want_curv=True), got, "chunks of 2, grad")
            assert ctx.last_trees_stats['n_launches'] == 3 * (5 if kw.get('generic') else 6)
    finally:
        CO.set_site_tile(0)


# ---- B. a workgroup that takes several items -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def compute_units():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked once and in a process of its own: PyTorch brings its own
    HIP runtime, which finds no device in a process that already holds the library's"""
    p = subprocess.run([sys.executable, '-c', 'import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)'],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return int(p.stdout.decode().split()[-1])


def strided_against_chunks(what, g, child, blen, Q, tile, sample, monkeypatch):
    """one call whose items exceed ptg_updown's grid against the same trees in chunks whose items fit under it (one item per
    workgroup: the path every other test takes), bit for bit; and against the restatement on the trees of `sample`"""
    N, S, T = g.shape[0], g.shape[1], child.shape[0]
    per_chunk = 6 if (((g == 0) | (g == 1)).all() and (g.sum(axis=2) >= 1).all()) else 5
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR, tile=tile) as ctx:
        ntiles = -(-S // ctx.site_tile())
        # min(items, 8 multiProcessorCount, 256 MiB / ((N-1) U 2 KiB)), U = 2: ptg_make_plan's grid
        cap = min(8 * compute_units(), (256 << 20) // ((N - 1) * 2 * 2048))
        items = T * ntiles
        assert cap == EC.updown_cap(N, compute_units()) and cap < items and items % cap != 0, (cap, items)
        for w in range(cap, items):                                       # (only where the set was built for it)
            if what.endswith('mixed'):
                assert child[w // ntiles].tobytes() != child[(w - cap) // ntiles].tobytes()
        full = ctx.trees_grad(child, blen, prior=PRIOR, want_curv=True)
        assert ctx.last_trees_stats['n_launches'] == per_chunk           # one chunk: items > grid, workgroups stride
        assert np.isfinite(full[0]).all()
        np.testing.assert_array_equal(bits(full[0]), bits(ctx.trees_loglik(child, blen, prior=PRIOR)))
        same_bits(ctx.trees_grad(child, blen, prior=PRIOR), full[:2], what + ": without curvature")
        rll, rgrad, rcurv, scale = reference(ctx, child[sample], blen[sample], Q, PRIOR, g)
        assert np.isfinite(rgrad).all() and np.isfinite(rcurv).all()      # (NaN below the floor: test_trees_edges_cpu.py holds the factors above 2^-1000)
        np.testing.assert_allclose(full[0][sample], rll, rtol=1e-12, atol=0)
        close(what + " grad", full[1][sample], rgrad, scale)
        close(what + " curv", full[2][sample], rcurv, scale)
    chunk = cap // ntiles
    assert chunk >= 1 and chunk * ntiles <= cap
    monkeypatch.setenv('PHYLO_TREES_CHUNK', str(chunk))
    with make_ctx(g, Q, pi=PRIOR, tile=tile) as ctx:
        parts = ctx.trees_grad(child, blen, prior=PRIOR, want_curv=True)
        assert ctx.last_trees_stats['n_launches'] == -(-T // chunk) * per_chunk
    same_bits(full, parts, what + ": strided against one item per workgroup")


@pytest.mark.parametrize("which", ['coded', 'generic', 'mixed'])
def test_strided_items_five_taxa(which, monkeypatch):
    cus = compute_units()
    T = EC.strided_T(5, 3, cus)
    if which == 'mixed':
        g, child, blen, Q = EC.small_mixed(T, EC.updown_cap(5, cus))
    else:
        g, child, blen, Q = EC.small_strided(T, generic=which == 'generic')
    assert (g.sum(axis=2) == 4).any()                                     # gaps
    cap = EC.updown_cap(5, cus)
    assert 3 * T >= cap + 5
    sample = sorted(set(range(8)) | set(range(0, T, 37)) | set(range(cap // 3 - 2, T)))      # ... and every tree of a second item
    strided_against_chunks('N5 ' + which, g, child, blen, Q, 64, sample, monkeypatch)


@pytest.mark.parametrize("which", ['same', 'mixed'])
def test_strided_items_512_taxa(which, monkeypatch):
    assert EC.updown_cap(512, compute_units()) == 128                     # the node store's share of the cap: 256 MiB / (511 2 2 KiB)
    g, child, blen, Q = EC.large_strided(which == 'mixed')
    sample = [0, 1, 2, 64, 127, 128, 129, 130]                            # the first, the 129th, the last
    strided_against_chunks('N512 ' + which, g, child, blen, Q, None, sample, monkeypatch)


# ---- C. the floor of the range: generic leaves scaled by exact powers of two ---------------------------------------------------
@pytest.fixture(scope="module")
def unscaled():
    g, child, blen, Q = EC.scaled_base()
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        assert ctx.site_tile() == 64
        got = ctx.trees_grad(child, blen, prior=PRIOR, want_curv=True)
        _, sites = ctx.trees_loglik(child, blen, prior=PRIOR, want_sites=True)
        ref = TR.trees_grad(child, device_matrices(ctx, blen), Q, PRIOR, g, want_sites=True)
    assert np.isfinite(got[0]).all() and (ref[4] > 2.0 ** -200).all()
    close("unscaled grad", got[1], ref[1], ref[3])
    close("unscaled curv", got[2], ref[2], ref[3])
    for a in got + (sites,) + ref:
        a.setflags(write=False)
    return g, child, blen, Q, got, sites, ref


@pytest.mark.parametrize("place", EC.PLACES)
def test_scaled_sites(place, unscaled):
    g, child, blen, Q, (ll0, grad0, curv0), sites0, (_, _, _, scale0, L0) = unscaled
    e = EC.scaled_exponents(place, L0)
    gs = EC.scaled_leaves(g, e)
    at = list(EC.SCALED_SITES)
    with make_ctx(gs, Q, pi=PRIOR, tile=64) as ctx:
        _, rgrad, rcurv, _, L = TR.trees_grad(child, device_matrices(ctx, blen), Q, PRIOR, gs, want_sites=True)
        print(place, "reference: scaled site factors in [%.3g, %.3g]" % (L[:, at].min(), L[:, at].max()))
        np.testing.assert_array_equal(np.delete(L, at, axis=1), np.delete(L0, at, axis=1))
        plain, sites = ctx.trees_loglik(child, blen, prior=PRIOR, want_sites=True)
        ll, grad, curv = ctx.trees_grad(child, blen, prior=PRIOR, want_curv=True)
        grad_only = ctx.trees_grad(child, blen, prior=PRIOR)
        np.testing.assert_array_equal(bits(ll), bits(plain), err_msg="loglik against phylo_trees_loglik")
        np.testing.assert_array_equal(bits(grad_only[0]), bits(plain))
        np.testing.assert_array_equal(bits(np.delete(sites, at, axis=1)), bits(np.delete(sites0, at, axis=1)))
        shift = e.sum() * np.log(2.0)
        if place == '2^-900':
            assert (L[:, at] < 2.0 ** -880).all() and (L[:, at] > 2.0 ** -960).all()
            np.testing.assert_array_equal(bits(sites[:, at]), bits(np.ldexp(sites0[:, at], -e[None, :])))
            np.testing.assert_array_equal(bits(grad), bits(grad0))
            np.testing.assert_array_equal(bits(curv), bits(curv0))
            np.testing.assert_array_equal(bits(grad_only[1]), bits(grad0))
            np.testing.assert_allclose(ll, ll0 - shift, rtol=1e-12, atol=0)
        elif place in EC.IN_RANGE:
            assert (L[:, at] >= FLOOR).all() and (L[:, at] <= ROOMY).all()
            if place == 'at-the-floor':
                assert (L[:, at].min(axis=0) < 2.0 ** -1019).all()
            assert np.isfinite(ll).all() and (sites[:, at] >= FLOOR).all()
            np.testing.assert_allclose(ll, ll0 - shift, rtol=1e-12, atol=0)
            close(place + " grad against the unscaled call", grad, grad0, scale0)
            close(place + " curv against the unscaled call", curv, curv0, scale0)
            close(place + " grad alone against the unscaled call", grad_only[1], grad0, scale0)
            close(place + " grad against the reference", grad, rgrad, scale0)
            close(place + " curv against the reference", curv, rcurv, scale0)
        else:
            assert (L[:, at] < FLOOR).all() and np.isnan(rgrad).all() and np.isnan(rcurv).all()
            if place == 'just-below':
                assert (L[:, at].max(axis=0) >= 2.0 ** -1021).all()
            if place == 'zero':
                assert (L[:, at] == 0).all() and (sites[:, at] == 0).all() and (ll == -np.inf).all()
            else:
                assert (L[:, at] > 0).all() and (sites[:, at] > 0).all() and (sites[:, at] < FLOOR).all() and np.isfinite(ll).all()
            assert np.isnan(grad).all() and np.isnan(curv).all() and np.isnan(grad_only[1]).all()


def test_one_site_below_the_floor_spoils_its_tree_alone():
    """a set in which only SOME trees see a factor below the floor: the others keep the bits they have without it"""
    g, child, blen, Q = EC.scaled_base()
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        _, _, _, scale0, L0 = TR.trees_grad(child, device_matrices(ctx, blen), Q, PRIOR, g, want_sites=True)
        want = ctx.trees_grad(child, blen, prior=PRIOR, want_curv=True)
    s = 129
    order = np.argsort(L0[:, s])
    e = int(np.frexp(L0[order[2], s])[1]) + 1020                          # the third smallest lands in [2^-1021, 2^-1020) ...
    gs = g.copy()
    gs[0, s], gs[1, s] = np.ldexp(g[0, s], -(e // 2)), np.ldexp(g[1, s], -(e - e // 2))
    with make_ctx(gs, Q, pi=PRIOR, tile=64) as ctx:
        L = TR.trees_site_factors(child, device_matrices(ctx, blen), PRIOR, gs)
        out = (L < FLOOR).any(axis=1)
        assert 1 <= out.sum() < out.size and (L > 0).all(), L[:, s]
        ll, grad, curv = ctx.trees_grad(child, blen, prior=PRIOR, want_curv=True)
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)))
        assert np.isfinite(ll).all()
        assert np.isnan(grad[out]).all() and np.isnan(curv[out]).all()
        close("in-range trees, grad", grad[~out], want[1][~out], scale0[~out])
        close("in-range trees, curv", curv[~out], want[2][~out], scale0[~out])


# ---- C. coded leaves: random columns over 300 and 310 taxa -----------------------------------------------------------------------
def test_300_taxa_random_columns_stay_in_range():
    g, child, blen, Q = EC.random_columns(300)
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        rll, rgrad, rcurv, scale, L = TR.trees_grad(child, device_matrices(ctx, blen), Q, PRIOR, g, want_sites=True)
        print("N = 300: smallest site factor per tree", L.min(axis=1))
        assert (L >= FLOOR).all() and L.min() < 1e-300
        ll, grad, curv = ctx.trees_grad(child, blen, prior=PRIOR, want_curv=True)
        dev, ora, _ = one_by_one(ctx, g, Q, PRIOR, child, blen)
        assert np.isfinite(ll).all()
        np.testing.assert_array_equal(bits(ll), bits(dev), err_msg="against phylo_tree_loglik")
        np.testing.assert_array_equal(bits(ll), bits(ora), err_msg="against the C oracle")
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)))
        np.testing.assert_allclose(ll, rll, rtol=1e-12, atol=0)
        close("N300 grad", grad, rgrad, scale)
        close("N300 curv", curv, rcurv, scale)


def test_310_taxa_random_columns_leave_the_range():
    """Trees 0 and 1 have subnormal site factors, none zero, and a finite loglik: before the floor rule phylo_trees_grad gave them
    inf and NaN beside numbers made from a few bits.  Tree 2 has a factor that is zero: loglik -inf, NaN by the older rule."""
    g, child, blen, Q = EC.random_columns(310)
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        rll, rgrad, rcurv, scale, L = TR.trees_grad(child, device_matrices(ctx, blen), Q, PRIOR, g, want_sites=True)
        out = (L < FLOOR).any(axis=1)
        print("N = 310: smallest site factor per tree", L.min(axis=1), "factors below the floor", (L < FLOOR).sum(axis=1), "loglik", rll)
        assert out.any() and out[0] and np.isfinite(rll[0]) and (L[0] > 0).all()
        ll, grad, curv = ctx.trees_grad(child, blen, prior=PRIOR, want_curv=True)
        print("device: loglik", ll, "derivative entries not NaN:", (~np.isnan(grad)).sum(axis=(1, 2)), (~np.isnan(curv)).sum(axis=(1, 2)))
        dev, _, _ = one_by_one(ctx, g, Q, PRIOR, child, blen)
        np.testing.assert_array_equal(bits(ll), bits(dev), err_msg="against phylo_tree_loglik")
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)))
        assert np.isfinite(ll[0])
        assert np.isnan(grad[out]).all() and np.isnan(curv[out]).all()
        if (~out).any():                                                  # a tree that stays in range: the reference
            close("N310 in-range grad", grad[~out], rgrad[~out], scale[~out])
            close("N310 in-range curv", curv[~out], rcurv[~out], scale[~out])
        with pytest.raises(OutOfRangeError, match="tree 0"):
            optimize_branches(lambda b: ctx.trees_grad(child, b, prior=PRIOR, want_curv=True), child, np.maximum(blen, 1e-8))
