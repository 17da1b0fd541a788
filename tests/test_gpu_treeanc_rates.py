"""phylo_trees_ancestral_rates on the device: the marginal posterior of every state at every internal node
and site of a set of trees under a mixture of rate categories, the most probable state and its posterior, every category's
posterior per site and the posterior mean rate of the site.  loglik is held to phylo_trees_loglik_rates' bits, catpost to that
call's own cat_lik and site_lik bit for bit, siterate, state and pmax to the device's own catpost and post bit for bit; post,
catpost and siterate to the NumPy restatement (treeanc_rates_ref.py, fed with the device's own branch matrices) within
TOL_ANC_RATES |value|, a bound set from the restatement's own error against 50-digit arithmetic (treeanc_rates_cases.py) before
the kernel ran.  Then: the same bits every way, a workgroup that takes several items, 129 and 512 taxa, the per-site NaN rule and
the near-floor allowance, refusals, what the call leaves alone, VCSMC.score_trees and runner.py --score_ancestral_rates.

Every test here needs Context.trees_ancestral_rates: AttributeError without it."""
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import treeanc_rates_cases as RC
import treeanc_rates_ref as ARR
import treegrad_edges_cases as GC
import trees_edges_cases as EC
from phylo_amd import _ffi
from phylo_amd import ancestral as A
from phylo_amd import rates as R
from phylo_amd import treepost as TP
from phylo_amd.datasets import load_dataset
from test_gpu_trees_edges import compute_units
from test_gpu_trees_loglik import PI, alignment, bits, gtr_Q, make_ctx, random_trees
from treeanc_rates_cases import MIX_I_G4, MIXTURES, PRIOR, TOL_ANC_RATES

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ALL = dict(want_post=True, want_state=True, want_pmax=True, want_catpost=True, want_siterate=True)
NAMES = ('post', 'state', 'pmax', 'catpost', 'siterate')


def device_matrices(ctx, blen, rates):
    """the device's own branch matrices of every category (ctx.expm_batched at rate[c] * blen, the host's one multiply): expm
    differences stay out of the comparison.  blen [T][N-1][2], rates [C] or [T][C]  ->  [T][C][N-1][2][4][4]"""
    blen, rates = np.asarray(blen), np.asarray(rates)
    r = np.broadcast_to(rates, (blen.shape[0], rates.shape[-1]))
    t = r[:, :, None, None] * blen[:, None]
    return ctx.expm_batched(t.reshape(-1)).reshape(t.shape + (4, 4))


def own_chains(got, rates, what):
    """state and pmax are map_states of the device's own post; siterate is the chain e = e + r_c catpost_c over the device's own
    catpost -- bit for bit"""
    ll, post, state, pmax, catpost, siterate = got
    st, pm = ARR.map_states(post)
    np.testing.assert_array_equal(state, st, err_msg=what + ": state against the device's own post")
    np.testing.assert_array_equal(bits(pmax), bits(pm), err_msg=what + ": pmax against the device's own post")
    assert state.dtype == np.uint8
    r = np.broadcast_to(np.asarray(rates), (post.shape[0], catpost.shape[1]))
    e = np.zeros(siterate.shape)
    with np.errstate(invalid='ignore'):
        for c in range(catpost.shape[1]):
            e = e + r[:, c, None] * catpost[:, c]
    np.testing.assert_array_equal(bits(siterate), bits(e), err_msg=what + ": siterate against the chain over the device's own catpost")


def own_catpost(ctx, child, blen, rates, weights, got, what, prior=PRIOR):
    """loglik is trees_loglik_rates' and catpost is (w_c cat_lik) (1 / site_lik) from that call's own outputs -- bit for bit"""
    rates, weights = np.asarray(rates), np.asarray(weights)
    T = len(child)
    for t in range(T) if rates.ndim == 2 else [slice(0, T)]:
        sel = slice(t, t + 1) if rates.ndim == 2 else t
        r, w = (rates[t], weights[t]) if rates.ndim == 2 else (rates, weights)
        ll, sites, cats = ctx.trees_loglik_rates(child[sel], blen[sel], r, w, prior=prior, want_sites=True, want_cats=True)
        np.testing.assert_array_equal(bits(got[0][sel]), bits(ll), err_msg=what + ": loglik against phylo_trees_loglik_rates")
        with np.errstate(all='ignore'):
            inv = np.where(np.isfinite(sites) & (sites >= ARR.FLOOR), 1.0 / sites, np.nan)
            want = (w[None, :, None] * cats) * inv[:, None, :]
        np.testing.assert_array_equal(bits(got[4][sel]), bits(want), err_msg=what + ": catpost against (w cat_lik) (1 / site_lik)")


def against_reference(what, ctx, child, blen, g, rates, weights, got, tol=None, allowance=False, prior=PRIOR):
    """post, catpost and siterate within the tolerance of the restatement, state and the most probable category equal to the
    restatement's wherever that is decided; prints the worst error per output; returns the restatement"""
    ll, post, state, pmax, catpost, siterate = got
    with GC.hardware_fma():
        ref = ARR.trees_ancestral_rates(child, device_matrices(ctx, blen, rates), prior, g, rates, weights, exact_mix=False)
    assert np.isfinite(ref['post']).all() and (ref['m'] >= ARR.FLOOR).all()
    np.testing.assert_allclose(ll, ref['loglik'], rtol=1e-12, atol=0)
    xp, xc, xr = RC.allowance(ref['m'], np.asarray(rates).reshape(-1, np.shape(rates)[-1])[0], np.asarray(weights).reshape(-1, np.shape(weights)[-1])[0]) \
        if allowance else (np.zeros(ref['m'].shape),) * 3
    worst = {}
    for key, val, extra in (('post', post, xp[:, None, :, None]), ('catpost', catpost, xc if allowance else 0.0), ('siterate', siterate, xr)):
        ok, worst[key] = RC.within(val, ref[key], extra, tol)
        assert np.isfinite(val).all() and ok.all(), (what, key, worst[key])
    same = float((bits(post) == bits(ref['post'])).mean())
    print("%s: worst |device - reference| in units of the bound: post %.3g, catpost %.3g, siterate %.3g (tolerance %.3g); %.2f %% of post "
          "bit-identical; worst |sum_j post - 1| = %.3g, |sum_c catpost - 1| = %.3g"
          % (what, worst['post'], worst['catpost'], worst['siterate'], TOL_ANC_RATES if tol is None else tol, 100 * same,
             np.abs(post.sum(axis=-1) - 1.0).max(), np.abs(catpost.sum(axis=1) - 1.0).max()))
    own_chains(got, rates, what)
    dec = RC.decided(ref['post'])
    assert 1.0 - float(dec.mean()) < RC.MAX_EXCLUDED, what
    np.testing.assert_array_equal(state[dec], ref['state'][dec], err_msg=what + ": state against the restatement")
    ok, w = RC.within(pmax[dec], ref['pmax'][dec], xp[:, None, :].repeat(post.shape[1], axis=1)[dec], tol)
    assert ok.all(), (what, 'pmax', w)
    dc = RC.decided(ref['catpost'], axis=-2)
    assert 1.0 - float(dc.mean()) < RC.MAX_EXCLUDED, what
    np.testing.assert_array_equal(A.category_states(catpost)[dc], A.category_states(ref['catpost'])[dc], err_msg=what + ": most probable category")
    return ref


def same_bits(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        if a.dtype == np.uint8:
            np.testing.assert_array_equal(a, b, err_msg="%s: output %d" % (what, k))
        else:
            np.testing.assert_array_equal(bits(a), bits(b), err_msg="%s: output %d" % (what, k))


# ---- 1. against the restatement: the smallest shapes, three chunks each ------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.CASES))
def test_against_the_reference(name, monkeypatch):
    g, Q, child, blen, jc, tile, rates, weights = RC.case_inputs(name)
    N, S, n, nc = g.shape[0], g.shape[1], len(child), rates.size
    monkeypatch.setenv('PHYLO_TREES_CHUNK', '3')                          # read when the context is created: chunks of 3, 3 and 1
    with make_ctx(g, Q, jc=jc, tile=tile) as ctx:
        got = ctx.trees_ancestral_rates(child, blen, rates, weights, prior=PRIOR, **ALL)
        st = ctx.last_trees_stats
        assert [a.shape for a in got] == [(n,), (n, N - 1, S, 4), (n, N - 1, S), (n, N - 1, S), (n, nc, S), (n, S)]
        assert st['units'] == n * S * (N - 1) * nc and st['sweep_ms'] > 0
        per_chunk = 3 if RC.CASES[name].get('generic') else 4             # expm, (coded leaves: the gap rows of M), ptar_updown, pt2_finish
        assert st['n_launches'] == 3 * per_chunk
        assert np.isfinite(got[0]).all()
        own_catpost(ctx, child, blen, rates, weights, got, name)
        against_reference(name, ctx, child, blen, g, rates, weights, got)
        rev = ctx.trees_ancestral_rates(child[::-1], blen[::-1], rates, weights, prior=PRIOR, **ALL)     # a tree's bits do not depend on its place
        same_bits([a[::-1] for a in rev], got, "the trees in reverse order")


def test_prior_none_is_the_models_pi():
    g = alignment(7, 70, 3, gaps=True)
    pi = np.array([0.4, 0.3, 0.2, 0.1])
    child, blen = random_trees(7, 9, 5)
    with make_ctx(g, gtr_Q(), pi=pi) as ctx:
        a, b = ctx.trees_ancestral_rates(child, blen, *MIX_I_G4), ctx.trees_ancestral_rates(child, blen, *MIX_I_G4, prior=pi)
        assert len(a) == 3                                               # the default: loglik, post, state
        same_bits(a, b, "prior None against the model's pi")
        assert not np.array_equal(a[1], ctx.trees_ancestral_rates(child, blen, *MIX_I_G4, prior=PI)[1])
        with pytest.raises(ValueError):
            ctx.trees_ancestral_rates(child, blen, *MIX_I_G4, want_post=False, want_state=False)
        with pytest.raises(ValueError):
            ctx.trees_ancestral_rates(child, blen, MIX_I_G4[0], MIX_I_G4[1][:4])
        with pytest.raises(ValueError):
            ctx.trees_ancestral_rates(child, blen, np.tile(MIX_I_G4[0], (4, 1)), np.tile(MIX_I_G4[1], (4, 1)))      # [T][C] with the wrong T


# ---- 2. bit contracts ------------------------------------------------------------------------------------------------------------------
def test_one_category_of_rate_one_is_trees_ancestral():
    """C = 1, rate 1, weight 1: 0 + 1 q = q and m = 1 f, so post, state and pmax are phylo_trees_ancestral's bits; catpost is
    f (1 / f) and siterate 1 * that.  Two categories of rate 1 and weight 1/2: printed, not asserted."""
    g = alignment(12, 130, 31, gaps=True)
    child, blen = random_trees(12, 6, 9)
    one = np.array([1.0])
    with make_ctx(g, gtr_Q(), tile=64) as ctx:
        plain = ctx.trees_ancestral(child, blen, prior=PRIOR, want_post=True, want_state=True, want_pmax=True)
        got = ctx.trees_ancestral_rates(child, blen, one, one, prior=PRIOR, **ALL)
        same_bits(got[:4], plain, "C = 1 against phylo_trees_ancestral")
        own_catpost(ctx, child, blen, one, one, got, "C = 1")
        own_chains(got, one, "C = 1")
        assert np.abs(got[4] - 1.0).max() <= 2.0 ** -52 and np.abs(got[5] - 1.0).max() <= 2.0 ** -52
        two = ctx.trees_ancestral_rates(child, blen, np.array([1.0, 1.0]), np.array([0.5, 0.5]), prior=PRIOR, **ALL)
        with np.errstate(invalid='ignore', divide='ignore'):
            rel = np.nanmax(np.abs(two[1] / got[1] - 1.0))
        print("two categories of rate 1 and weight 1/2 against one: %.2f %% of post bit-identical, worst relative difference %.3g; loglik %s"
              % (100 * float((bits(two[1]) == bits(got[1])).mean()), rel,
                 'equal' if np.array_equal(bits(two[0]), bits(got[0])) else 'not equal'))


# ---- 3. the same bits every way ----------------------------------------------------------------------------------------------------------
def test_same_bits_every_way(monkeypatch):
    g = alignment(12, 130, 31, gaps=True)
    child, blen = random_trees(12, 6, 11)
    rates, weights = MIX_I_G4
    n = len(child)
    got = {}
    for chunk in ('0', '4'):
        monkeypatch.setenv('PHYLO_TREES_CHUNK', chunk)
        with make_ctx(g, gtr_Q(), tile=64) as ctx:
            got[chunk] = ctx.trees_ancestral_rates(child, blen, rates, weights, **ALL)
            assert ctx.last_trees_stats['n_launches'] == 4 * {'0': 1, '4': 3}[chunk]
            same_bits(ctx.trees_ancestral_rates(child, blen, rates, weights, **ALL), got[chunk], "a second call")
            if chunk == '4':
                rev = ctx.trees_ancestral_rates(child[::-1], blen[::-1], rates, weights, **ALL)
                same_bits([a[::-1] for a in rev], got[chunk], "the set reversed")
                per = ctx.trees_ancestral_rates(child, blen, np.tile(rates, (n, 1)), np.tile(weights, (n, 1)), **ALL)
                same_bits(per, got[chunk], "[T][C] against [C] with the same numbers")
                sets = [(k,) for k in range(5)] + [(1, 4), (0, 1, 2, 3, 4)]     # each output alone, (state, siterate), all five
                for s in sets:
                    flags = {'want_' + NAMES[k]: k in s for k in range(5)}
                    part = ctx.trees_ancestral_rates(child, blen, rates, weights, **flags)
                    same_bits(part, [got[chunk][0]] + [got[chunk][1 + k] for k in s], "outputs %r" % (s,))
                # every tree under its own alpha (and p_inv): one per-tree call against T single-tree calls
                mixes = [R.rate_model(0.3 + 0.2 * t, 4, 0.02 * t, keep_invariant=True) for t in range(n)]
                r_t, w_t = np.array([m[0] for m in mixes]), np.array([m[1] for m in mixes])
                assert r_t.shape == (n, 5) and len(set(r_t[:, 2].tolist())) == n
                per = ctx.trees_ancestral_rates(child, blen, r_t, w_t, **ALL)
                for t in range(n):
                    single = ctx.trees_ancestral_rates(child[t:t + 1], blen[t:t + 1], r_t[t], w_t[t], **ALL)
                    same_bits(single, [a[t:t + 1] for a in per], "tree %d under its own mixture" % t)
                own_catpost(ctx, child, blen, r_t, w_t, per, "per-tree mixtures", prior=None)
                own_chains(per, r_t, "per-tree mixtures")
    same_bits(got['4'], got['0'], "three chunks against one")


def test_strided_items(monkeypatch):
    """N = 5, S = 192 in tiles of 64 (three tiles), T trees with 3 T = 8 CUs + 5 items (or the next multiple of three above) on
    the 8 CUs workgroups of the capped grid: some workgroups take a second item, of another tree, and write the planes of their
    node store again -- against the same trees in chunks of one item per workgroup"""
    cus = compute_units()
    cap = 8 * cus
    rates, weights = MIX_I_G4
    assert cap <= (256 << 20) // (rates.size * 4 * 2 * 2048)              # the compute units, not the node stores, cap the grid
    n = -(-(cap + 5) // 3)
    g = alignment(5, 192, 77, gaps=True)
    child, blen = random_trees(5, 78, n)
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, gtr_Q(), pi=PRIOR, tile=64) as ctx:
        assert -(-192 // ctx.site_tile()) == 3 and 3 * n > cap and (3 * n) % cap != 0
        full = ctx.trees_ancestral_rates(child, blen, rates, weights, **ALL)
        assert ctx.last_trees_stats['n_launches'] == 4                   # one chunk: items > grid, workgroups stride
        sample = sorted(set(range(4)) | set(range(cap // 3 - 2, n)))      # the first trees, and every tree of a second item
        sub = [a[sample] for a in full]
        own_catpost(ctx, child[sample], blen[sample], rates, weights, sub, "strided")
        against_reference("strided", ctx, child[sample], blen[sample], g, rates, weights, sub)
    chunk = cap // 3
    monkeypatch.setenv('PHYLO_TREES_CHUNK', str(chunk))
    with make_ctx(g, gtr_Q(), pi=PRIOR, tile=64) as ctx:
        parts = ctx.trees_ancestral_rates(child, blen, rates, weights, **ALL)
        assert ctx.last_trees_stats['n_launches'] == -(-n // chunk) * 4
    same_bits(full, parts, "strided against one item per workgroup")


# ---- 4. 512 and 129 taxa ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.E_REF_BIG))
def test_many_taxa(name, monkeypatch):
    """caterpillar-N512 and balanced-N512 (the 9-slot schedule) under 16 categories: 32 MiB of node store per workgroup, so 8
    workgroups walk the 10 items of five trees in tiles of 64; balanced-N129 at S = 130 in tiles of 64 under MIX_I_G4.  Held to
    8 max(E_REF_ANC_RATES, E_REF_BIG) 2^-53, the restatement's own 50-digit error on these trees, and the absolute allowance
    for a category whose own terms are subnormal beside an m in range (treeanc_rates_cases.py)"""
    g, child, blen, Q, rates, weights, tile = RC.big_case(name)
    N, S, n = g.shape[0], g.shape[1], len(child)
    depth = max(_ffi.debug_tree_schedule(c, b)[1] for c, b in zip(child, blen))
    assert depth == {'caterpillar-N512': 1, 'balanced-N512': 9, 'balanced-N129-S130': 7}[name]
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR, tile=tile) as ctx:
        got = ctx.trees_ancestral_rates(child, blen, rates, weights, **ALL)
        ntiles = -(-S // 64)
        assert ctx.last_trees_stats['n_launches'] == 4 and ctx.last_trees_stats['units'] == n * S * (N - 1) * rates.size
        if N == 512:
            assert n * ntiles == 10 and (256 << 20) // (16 * 511 * 2 * 2048) == 8      # 10 items on 8 workgroups
        own_catpost(ctx, child, blen, rates, weights, got, name)
        against_reference(name, ctx, child, blen, g, rates, weights, got, tol=RC.tol_big(name), allowance=True)


# ---- 5. the NaN rule, per site; the near-floor allowance -----------------------------------------------------------------------------------
def test_nan_rule_is_per_site():
    g, child, blen, Q = EC.scaled_base()
    rates, weights = MIX_I_G4
    S = g.shape[1]
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        base = ctx.trees_ancestral_rates(child, blen, rates, weights, **ALL)
        m0 = ctx.trees_loglik_rates(child, blen, rates, weights, want_sites=True)[1]
    assert np.isfinite(base[1]).all() and (m0 > 2.0 ** -200).all()
    e = EC.scaled_exponents('just-below', m0)
    for k, s in enumerate(EC.SCALED_SITES):                               # ONE site just below the floor: each of the four in turn
        only = np.where(np.arange(len(e)) == k, e, 0)
        gs = EC.scaled_leaves(g, only)
        others = [x for x in range(S) if x != s]
        with make_ctx(gs, Q, pi=PRIOR, tile=64) as ctx:
            ll, post, state, pmax, catpost, siterate = got = ctx.trees_ancestral_rates(child, blen, rates, weights, **ALL)
            scored, sites = ctx.trees_loglik_rates(child, blen, rates, weights, want_sites=True)
            own_catpost(ctx, child, blen, rates, weights, got, "site %d below the floor" % s, prior=None)
        assert (sites[:, s] < ARR.FLOOR).all() and (sites[:, s] > 0).all() and (sites[:, others] >= 2.0 ** -200).all()
        np.testing.assert_array_equal(bits(ll), bits(scored), err_msg="loglik stays the scoring call's")
        assert np.isfinite(ll).all()
        assert np.isnan(post[:, :, s]).all() and (state[:, :, s] == _ffi.ANC_NOSTATE).all() and np.isnan(pmax[:, :, s]).all()
        assert np.isnan(catpost[:, :, s]).all() and np.isnan(siterate[:, s]).all()
        same_bits([post[:, :, others], state[:, :, others], pmax[:, :, others], catpost[:, :, others], siterate[:, others]],
                  [base[1][:, :, others], base[2][:, :, others], base[3][:, :, others], base[4][:, :, others], base[5][:, others]],
                  "site %d below the floor: every other column" % s)


@pytest.mark.parametrize("place", EC.IN_RANGE)
def test_in_range_at_the_floor(place):
    """the four scaled sites with m at 2^-900, at the floor and inside [2^-1020, 2^-1000): nothing is NaN, every other column
    keeps its bits, and the scaled columns stay within TOL_ANC_RATES and the counted allowance k 2^-1075 / m_s of the restatement
    (under the hardware fma, as section 13b restates scaled alignments)"""
    g, child, blen, Q = EC.scaled_base()
    rates, weights = MIX_I_G4
    at = list(EC.SCALED_SITES)
    others = [x for x in range(g.shape[1]) if x not in at]
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        base = ctx.trees_ancestral_rates(child, blen, rates, weights, **ALL)
        m0 = ctx.trees_loglik_rates(child, blen, rates, weights, want_sites=True)[1]
    gs = EC.scaled_leaves(g, EC.scaled_exponents(place, m0))
    with make_ctx(gs, Q, pi=PRIOR, tile=64) as ctx:
        got = ctx.trees_ancestral_rates(child, blen, rates, weights, **ALL)
        own_catpost(ctx, child, blen, rates, weights, got, place, prior=None)
        against_reference(place, ctx, child, blen, gs, rates, weights, got, allowance=place != '2^-900')
    same_bits([got[1][:, :, others], got[2][:, :, others], got[3][:, :, others], got[4][:, :, others], got[5][:, others]],
              [base[1][:, :, others], base[2][:, :, others], base[3][:, :, others], base[4][:, :, others], base[5][:, others]],
              place + ": every other column")


def test_nan_rule_generic_zero_row():
    N, S = 5, 70
    g = alignment(N, S, 22, generic=True)
    child, blen = random_trees(N, 4, 3)
    rates, weights = MIX_I_G4
    with make_ctx(g, gtr_Q()) as ctx:
        base = ctx.trees_ancestral_rates(child, blen, rates, weights, prior=PI, **ALL)
    g2 = g.copy()
    g2[2, 66] = 0.0                                                       # a generic leaf row of zeros kills the site in every tree
    others = [x for x in range(S) if x != 66]
    with make_ctx(g2, gtr_Q()) as ctx:
        ll, post, state, pmax, catpost, siterate = ctx.trees_ancestral_rates(child, blen, rates, weights, prior=PI, **ALL)
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik_rates(child, blen, rates, weights, prior=PI)))
    assert (ll == -np.inf).all()
    assert np.isnan(post[:, :, 66]).all() and (state[:, :, 66] == 255).all() and np.isnan(pmax[:, :, 66]).all()
    assert np.isnan(catpost[:, :, 66]).all() and np.isnan(siterate[:, 66]).all()
    same_bits([post[:, :, others], state[:, :, others], pmax[:, :, others], catpost[:, :, others], siterate[:, others]],
              [base[1][:, :, others], base[2][:, :, others], base[3][:, :, others], base[4][:, :, others], base[5][:, others]],
              "every other column")


# ---- 6. what the call leaves alone ---------------------------------------------------------------------------------------------------------
def test_siblings_scratch_is_left_alone():
    g = alignment(6, 70, 8, gaps=True)
    child, blen = random_trees(6, 3, 7)
    rates, weights = MIX_I_G4
    with make_ctx(g, gtr_Q()) as ctx:
        ll, sites = ctx.trees_loglik_rates(child, blen, rates, weights, want_sites=True)
        rl = ctx.rell(sites, 50, 3, want_reps=True)
        tg = ctx.trees_grad_rates(child, blen, rates, weights, want_curv=True, want_params=True)
        nn = ctx.trees_nni_rates(child, blen, rates, weights)
        an = ctx.trees_ancestral(child, blen, want_pmax=True)
        got = ctx.trees_ancestral_rates(child, blen, rates, weights, **ALL)
        np.testing.assert_array_equal(bits(got[0]), bits(ll))
        assert np.isfinite(got[1]).all() and (got[2] < 4).all()
        np.testing.assert_array_equal(bits(ctx.trees_loglik_rates(child, blen, rates, weights, want_sites=True)[1]), bits(sites))
        np.testing.assert_array_equal(bits(ctx.rell(sites, 50, 3, want_reps=True)['rep_loglik']), bits(rl['rep_loglik']))
        same_bits(ctx.trees_grad_rates(child, blen, rates, weights, want_curv=True, want_params=True), tg, "trees_grad_rates afterwards")
        same_bits(ctx.trees_nni_rates(child, blen, rates, weights), nn, "trees_nni_rates afterwards")
        same_bits(ctx.trees_ancestral(child, blen, want_pmax=True), an, "trees_ancestral afterwards")
        same_bits(ctx.trees_ancestral_rates(child, blen, rates, weights, **ALL), got, "and the call itself")


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing():
    N, S = 5, 70
    g = alignment(N, S, 41)
    child, blen = random_trees(N, 8, 4)
    child[2] = np.array([[0, 1], [2, 3], [6, 4], [5, 7]], dtype=np.int32)
    rates, weights = MIX_I_G4
    with _ffi.Context(4, N, S) as ctx:
        with pytest.raises(_ffi.PhyloError) as e:
            ctx.trees_ancestral_rates(child, blen, rates, weights)
        assert e.value.code == -6
        ctx.set_leaves(g)
        ctx.set_model(gtr_Q(), PI, np.full(N - 1, 10.0), np.full(N - 1, 10.0))
        ref = ctx.trees_ancestral_rates(child, blen, rates, weights, **ALL)

        def refused(call, what):
            with pytest.raises(_ffi.PhyloError) as e:
                call()
            assert e.value.code == -1 and what in str(e.value), str(e.value)
            same_bits(ctx.trees_ancestral_rates(child, blen, rates, weights, **ALL), ref, "a valid call after a refusal")

        c = child.copy(); c[2, 2] = [6, 0]
        refused(lambda: ctx.trees_ancestral_rates(c, blen, rates, weights), 'tree 2, row 2')        # a leaf used twice
        for v in (np.nan, -1e-9, np.inf):
            b = blen.copy(); b[2, 1, 1] = v
            refused(lambda: ctx.trees_ancestral_rates(child, b, rates, weights), 'tree 2, row 1')   # a negative (or non-finite) length
            r = np.tile(rates, (4, 1)); r[3, 2] = v
            refused(lambda: ctx.trees_ancestral_rates(child, blen, r, np.tile(weights, (4, 1))), 'tree 3: rate')
            w = weights.copy(); w[4] = v
            refused(lambda: ctx.trees_ancestral_rates(child, blen, rates, w), 'category 4')
        big = rates.copy(); big[4] = 1e300
        b = blen.copy(); b[1, 3, 0] = 1e10
        refused(lambda: ctx.trees_ancestral_rates(child, b, big, weights), 'tree 1: row 3, category 4')   # a scaled length that is not finite
        refused(lambda: ctx.trees_ancestral_rates(child, blen, np.ones(17), np.full(17, 1 / 17)), 'C=17')
        ch, bl = np.ascontiguousarray(child, dtype=np.int32), np.ascontiguousarray(blen)
        ll, st = np.empty(4), np.empty((4, N - 1, S), dtype=np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        raw = lambda *a: ctx._check(ctx._lib.phylo_trees_ancestral_rates(ctx._h, *a))
        head = (C.c_int(4), p(ch), p(bl), C.c_int(5), p(rates), p(weights))
        refused(lambda: raw(*head, C.c_int(0), None, p(ll), None, None, None, None, None, None), 'all five')
        refused(lambda: raw(*head, C.c_int(0), None, None, None, p(st), None, None, None, None), 'NULL')          # NULL loglik
        refused(lambda: raw(*head, C.c_int(2), None, p(ll), None, p(st), None, None, None, None), 'per_tree')
        refused(lambda: raw(C.c_int(0), *head[1:], C.c_int(0), None, p(ll), None, p(st), None, None, None, None), 'T >= 1')
        refused(lambda: raw(C.c_int(4), p(ch), p(bl), C.c_int(0), p(rates), p(weights), C.c_int(0), None, p(ll), None, p(st), None, None, None, None), 'C=0')
        refused(lambda: raw(C.c_int(4), p(ch), p(bl), C.c_int(5), None, p(weights), C.c_int(0), None, p(ll), None, p(st), None, None, None, None), 'NULL')
        with pytest.raises(ValueError):
            ctx.trees_ancestral_rates(child[:, :3], blen[:, :3], rates, weights)


def test_reuse_keeps_its_bits_across_contexts():
    g = alignment(12, 300, 9, gaps=True)
    child, blen = random_trees(12, 3, 8)
    first = None
    for _ in range(3):
        with make_ctx(g, gtr_Q()) as ctx:
            for _ in range(2):
                got = ctx.trees_ancestral_rates(child, blen, *MIXTURES['C16'], **ALL)
                first = got if first is None else first
                same_bits(got, first, "a fresh context, a second call")


# ---- 8. VCSMC.score_trees(ancestral_rates=k) and the runner ------------------------------------------------------------------------------------
def runner_files(argv, newicks, extra, tmp):
    path = os.path.join(tmp, 'trees.nwk')
    with open(path, 'w') as f:
        f.write('\n'.join(newicks) + '\n')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'runner.py')] + argv + ['--score_trees', path] + extra, cwd=tmp,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    (res,) = glob.glob(os.path.join(tmp, 'results', '*', '*', '*', '*', 'tree_scores.json'))
    here = os.path.dirname(res)
    files = {}
    for name in sorted(os.listdir(here)):
        if name.endswith(('.json', '.nwk', '.txt', '.fa', '.tre', '.tsv')):
            with open(os.path.join(here, name), 'rb') as f:
                files[name] = f.read().replace(tmp.encode(), b'TMP')       # (run_parameters.txt names the tree file's path)
    return files


def test_score_trees_ancestral_rates_keyword():
    """VCSMC.score_trees(rates=..., ancestral_rates=k): the k best trees under the mixture given, against a direct call; the
    keyword needs rates, and ancestral= keeps its ValueError with rates"""
    from phylo_amd.vcsmc import VCSMC, default_args
    N, S = 7, 70
    g = alignment(N, S, 3, gaps=True)
    taxa = ['t%d' % i for i in range(N)]
    child, blen = random_trees(N, 9, 5)
    blen = blen + 0.03
    newicks = [TP.rows_to_newick(c, b, taxa) for c, b in zip(child, blen)]
    spec = R.parse_spec('gamma:0.7:4:0.05')
    v = VCSMC({'taxa': taxa, 'genome': g}, K=4, args=default_args())
    try:
        with pytest.raises(ValueError):
            v.score_trees(newicks, ancestral_rates=2)                     # needs rates
        with pytest.raises(ValueError, match='not built for mixtures'):
            v.score_trees(newicks, rates=spec, ancestral=2)
        with pytest.raises(ValueError):
            v.score_trees(newicks, rates=spec, ancestral=2, ancestral_rates=2)
        scores = v.score_trees(newicks, rates=spec)
        assert v.last_ancestral is None
        again = v.score_trees(newicks, rates=spec, ancestral_rates=2)
        assert again == scores
        res = v.last_ancestral
        order = np.argsort(-np.array(scores), kind='stable')[:2]
        assert res['trees'] == [int(t) for t in order] and res['alpha'] is None and res['pinv'] is None
        assert res['catpost'].shape == (2, 5, S) and res['siterate'].shape == (2, S) and res['state'].shape == (2, N - 1, S)
        np.testing.assert_array_equal(res['rates'], np.tile(spec['rates'], (2, 1)))
        rows = [TP.newick_to_rows(nw, taxa) for nw in newicks]
        c2, b2 = np.array([rows[t][0] for t in order]), np.array([rows[t][1] for t in order])
        want = v._context().trees_ancestral_rates(c2, b2, spec['rates'], spec['weights'], want_post=False, want_pmax=True, want_catpost=True,
                                                  want_siterate=True)
        same_bits([np.array(res['loglik']), res['state'], res['pmax'], res['catpost'], res['siterate']], want, "score_trees against a direct call")
        # with a fit every tree is reconstructed under its own fitted alpha
        v.score_trees(newicks, rates=spec, optimize=True, fit=('alpha',), ancestral_rates=5)
        res = v.last_ancestral
        assert len(set(res['alpha'])) == 5 and res['rates'].shape == (5, 5) and len(set(res['rates'][:, 2].tolist())) == 5
        assert np.isfinite(res['siterate']).all() and np.abs(res['catpost'].sum(axis=1) - 1.0).max() < 1e-12
    finally:
        v.close()


def test_runner_score_ancestral_rates():
    d = load_dataset('primate_data_wang')                               # primates_small.fa: N = 9, S = 738
    taxa = [str(t) for t in d['taxa']]
    g = d['genome']
    N, S = g.shape[0], g.shape[1]
    child, blen = random_trees(N, 12, 3)
    blen = blen + 0.02
    newicks = [TP.rows_to_newick(c, b, taxa) for c, b in zip(child, blen)]
    argv = ['--dataset', 'primate_data_wang', '--n_particles', '16', '--num_epoch', '1', '--batch_size', '512', '--jcmodel', 'true',
            '--seed', '2', '--score_rates', 'gamma:0.5:4:0.1', '--score_fit', 'branches+alpha']
    with tempfile.TemporaryDirectory() as tmp:
        with_flag = runner_files(argv, newicks, ['--score_ancestral_rates', '2'], tmp)
    with tempfile.TemporaryDirectory() as tmp:
        without = runner_files(argv, newicks, [], tmp)
    # without the flag: no new file, no key; every other file byte for byte
    assert not {'ancestral.fa', 'ancestral.json', 'site_rates.tsv'} & set(without)
    assert b'score_ancestral_rates' not in without['run_parameters.txt'] and b'score_ancestral_rates : 2\n' in with_flag['run_parameters.txt']
    assert with_flag['run_parameters.txt'].replace(b'score_ancestral_rates : 2\n', b'') == without['run_parameters.txt']
    assert set(with_flag) == set(without) | {'ancestral.fa', 'ancestral.json', 'site_rates.tsv'}
    for name in without:
        if name != 'run_parameters.txt':
            assert with_flag[name] == without[name], name
    scores = json.loads(with_flag['tree_scores.json'])
    res = json.loads(with_flag['ancestral.json'])
    order = np.argsort(-np.array([t['loglik_ml'] for t in scores['trees']]), kind='stable')[:2]
    assert [t['tree'] for t in res['trees']] == [int(t) for t in order]
    records = {}
    for line in with_flag['ancestral.fa'].decode().splitlines():
        if line.startswith('>'):
            head = line[1:]
            records[head] = ''
        else:
            records[head] += line
    assert len(records) == 2 * (N - 1)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'site_rates.tsv')
        with open(path, 'wb') as f:
            f.write(with_flag['site_rates.tsv'])
        table = A.read_site_rates(path)
    assert table['trees'].tolist() == [int(t) for t in order] and table['siterate'].shape == (2, S) and table['catpost'].shape == (2, 5, S)
    # ... against a direct call under the model, the lengths and the fitted mixture the files name
    ml = with_flag['trees_ml.nwk'].decode().split()
    m = scores['model']
    with _ffi.Context(4, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(np.array(m['Q']), np.array(m['pi']), np.full(N - 1, 10.0), np.full(N - 1, 10.0), jc69_closed_form=m['jc69_closed_form'])
        for k, tree in enumerate(res['trees']):
            assert tree['newick'] == ml[tree['tree']]
            scored = scores['trees'][tree['tree']]
            assert tree['alpha'] == scored['alpha'] != 0.5 and tree.get('pinv') == scored.get('pinv') == 0.1
            r, w = np.array(tree['rates']), np.array(tree['weights'])                     # the mixture used: the tree's fitted alpha
            np.testing.assert_allclose(r, R.rate_model(tree['alpha'], 4, 0.1)[0], rtol=1e-12)
            np.testing.assert_allclose(w, R.rate_model(tree['alpha'], 4, 0.1)[1], rtol=1e-12)
            c, b = TP.newick_to_rows(tree['newick'], taxa)
            ll, state, pmax, catpost, siterate = ctx.trees_ancestral_rates(c[None], b[None], r, w, want_post=False, want_pmax=True,
                                                                           want_catpost=True, want_siterate=True)
            assert ll[0] == pytest.approx(tree['loglik'], rel=1e-12)
            np.testing.assert_allclose(table['siterate'][k], siterate[0], rtol=1e-9)      # (the Newick string rounds the lengths)
            np.testing.assert_allclose(table['catpost'][k], catpost[0], rtol=1e-9, atol=1e-300)
            sr = A.summarise_rates(siterate, catpost)
            assert tree['site_rates']['mean_rate'] == pytest.approx(float(sr['mean_rate'][0]), rel=1e-9)
            assert tree['site_rates']['n_nan'] == 0 and len(tree['site_rates']['category_share']) == 5
            assert sum(tree['site_rates']['category_share']) == pytest.approx(1.0)
            seqs = A.sequences(state[0])
            by_clade = {tuple(cl): i for i, cl in enumerate(A.node_clades(c, taxa))}
            for node in tree['nodes']:
                i = by_clade[tuple(node['clade'])]
                assert node['n_nan'] == 0
                assert records['tree%d_node%d clade=%s' % (tree['tree'], node['node'], ','.join(node['clade']))] == seqs[i]
