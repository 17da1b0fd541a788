"""phylo_trees_grad_rates on the device where test_gpu_treegrad_rates.py stops (inputs:
treegrad_edges_cases.py and trees_edges_cases.py).  A: items of several strips under the default site tile, so that the LDS
sums acc, dr and dw are carried from strip to strip, the node-store planes are written again, and a half-full second site step
runs beside live neighbours.  B: 129 to 512 taxa in every shape -- schedules of 1 to 9 slots, 511 dependent levels of the
downward pass --, and 512 taxa under 16 categories.  D: site values near the floor of the double range: below 2^-1020 every
derivative of the tree is NaN beside phylo_trees_loglik_rates' loglik bits; at and above it grad and curv are those of the
unscaled alignment within TOL_RATES, drate and dweight within section 13b's near-floor bound (treegrad_edges_cases.floor_excess).

ptgr_updown is a kernel of its own; what test_gpu_trees_edges.py shows of ptg_updown says nothing about it.  Every
precondition is asserted from the NumPy restatement (fed with the device's branch matrices) before anything is compared."""
import functools

import numpy as np
import pytest

import treegrad_edges_cases as GC
import trees_edges_cases as EC
from test_gpu_treegrad_rates import close, close_all, reference, same_bits
from test_gpu_trees_loglik import alignment, gtr_Q, make_ctx, random_trees
from treegrad_rates_cases import MIX_I_G4
from trees_edges_cases import FLOOR, PRIOR, ROOMY

pytestmark = pytest.mark.gpu
FULL = dict(prior=PRIOR, want_curv=True, want_params=True)


def bit_identities(ctx, child, blen, rates, weights, full, what):
    """the reversed set, the calls without curvature and without the parameters' derivatives: the bits of the full call"""
    rev = ctx.trees_grad_rates(child[::-1], blen[::-1], rates, weights, **FULL)
    same_bits([a[::-1] for a in rev], full, what + ": the set reversed")
    same_bits(ctx.trees_grad_rates(child, blen, rates, weights, prior=PRIOR), full[:2], what + ": grad alone")
    same_bits(ctx.trees_grad_rates(child, blen, rates, weights, prior=PRIOR, want_params=True), (full[0], full[1], full[3], full[4]),
              what + ": without curvature")
    same_bits(ctx.trees_grad_rates(child, blen, rates, weights, prior=PRIOR, want_curv=True), full[:3], what + ": without params")


# ---- A. one item of several strips -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GC.STRIPS))
def test_strips(name, monkeypatch):
    kw = GC.STRIPS[name]
    N, S = kw['N'], kw['S']
    rates, weights = GC.MIXTURES[kw['mix']]
    g = alignment(N, S, 100 + N + S, kw.get('gaps', False), kw.get('generic', False))
    Q = gtr_Q()
    child, blen = random_trees(N, 5, GC.T_STRIPS)
    assert (blen == 0).any()                                              # trees with zero-length branches
    per_chunk = 5 if kw.get('generic') else 6
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        assert ctx.site_tile() >= S                                       # the default tile: one item of ceil(S / 128) strips
        got = ctx.trees_grad_rates(child, blen, rates, weights, **FULL)
        assert ctx.last_trees_stats['n_launches'] == per_chunk
        same_bits([got[0]], [ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR)], "loglik against phylo_trees_loglik_rates")
        assert np.isfinite(got[0]).all()
        ref = reference(ctx, child, blen, Q, PRIOR, g, rates, weights)
        close_all("%s (%d strips)" % (name, -(-S // 128)), got, ref)
        same_bits(ctx.trees_grad_rates(child, blen, rates, weights, **FULL), got, "the call again")
        bit_identities(ctx, child, blen, rates, weights, got, name)
    monkeypatch.setenv('PHYLO_TREES_CHUNK', '2')                          # read when the context is created
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        same_bits(ctx.trees_grad_rates(child, blen, rates, weights, **FULL), got, "chunks of 2")
        assert ctx.last_trees_stats['n_launches'] == -(-GC.T_STRIPS // 2) * per_chunk


# ---- B. 129 to 512 taxa ------------------------------------------------------------------------------------------------------------
def many_taxa(name, mix, sample, chunks, monkeypatch):
    kw = EC.BIG[name]
    tile = kw.get('tile')
    g, child, blen, Q = EC.big_case(name)
    n = child.shape[0]
    rates, weights = mix
    per_chunk = 5 if kw.get('generic') else 6
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR, tile=tile) as ctx:
        ref = reference(ctx, child[sample], blen[sample], Q, PRIOR, g, rates, weights)
        assert (ref['m'] >= ROOMY).all()                                  # the precondition, before anything is compared
        assert -(-kw['S'] // ctx.site_tile()) == (3 if tile else 1)
        got = ctx.trees_grad_rates(child, blen, rates, weights, **FULL)
        st = ctx.last_trees_stats
        assert st['units'] == n * kw['S'] * (kw['N'] - 1) * rates.size and st['n_launches'] == per_chunk
        same_bits([got[0]], [ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR)], "loglik against phylo_trees_loglik_rates")
        assert np.isfinite(got[0]).all()
        GC.close_all_big("%s C%d" % (name, rates.size), [a[sample] for a in got], ref)
        bit_identities(ctx, child, blen, rates, weights, got, name)
    if chunks:
        monkeypatch.setenv('PHYLO_TREES_CHUNK', '2')
        with make_ctx(g, Q, pi=PRIOR, tile=tile) as ctx:
            same_bits(ctx.trees_grad_rates(child, blen, rates, weights, **FULL), got, "chunks of 2")
            assert ctx.last_trees_stats['n_launches'] == 3 * per_chunk


@pytest.mark.parametrize("name", list(EC.BIG))
def test_many_taxa(name, monkeypatch):
    many_taxa(name, MIX_I_G4, [0, 2], True, monkeypatch)


@pytest.mark.parametrize("name", ['generic-balanced-N512', 'caterpillar-N512'])
def test_512_taxa_16_categories(name, monkeypatch):
    """the LDS maximum and the deepest recursion together; 32 MiB of node store per workgroup"""
    assert GC.C16[0].size == 16
    many_taxa(name, GC.C16, [2], False, monkeypatch)


# ---- D. the floor of the range ------------------------------------------------------------------------------------------------------
FLOOR_MIXES = {'I+G4': MIX_I_G4, 'slow-fast': GC.MIX_SLOW_FAST}


@functools.lru_cache(maxsize=None)
def unscaled(mix):
    g, child, blen, Q = EC.scaled_base()
    rates, weights = FLOOR_MIXES[mix]
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        assert ctx.site_tile() == 64
        got = ctx.trees_grad_rates(child, blen, rates, weights, **FULL)
        ref = reference(ctx, child, blen, Q, PRIOR, g, rates, weights)
    assert np.isfinite(got[0]).all() and (ref['m'] > 2.0 ** -200).all()
    close_all("unscaled " + mix, got, ref)
    for a in got + tuple(ref.values()):
        a.setflags(write=False)
    return g, child, blen, Q, got, ref


def all_nan(arrays):
    return all(np.isnan(a).all() for a in arrays)


@pytest.mark.parametrize("place,mix", [(p, 'I+G4') for p in EC.PLACES] + [('at-the-floor', 'slow-fast')])
def test_scaled_sites(place, mix):
    g, child, blen, Q, got0, ref0 = unscaled(mix)
    rates, weights = FLOOR_MIXES[mix]
    e = EC.scaled_exponents(place, ref0['m'])                             # m in place of L: the rule is on the mixture value
    gs = EC.scaled_leaves(g, e)
    at = list(EC.SCALED_SITES)
    with make_ctx(gs, Q, pi=PRIOR, tile=64) as ctx:
        with GC.hardware_fma():                                           # the emulated fma is not the device's below 1e-290
            ref = reference(ctx, child, blen, Q, PRIOR, gs, rates, weights)
        m, f = ref['m'][:, at], ref['f'][:, :, at]
        print(place, mix, "reference: scaled site values in [2^%.1f, 2^%.1f], %d subnormal category factors"
              % (np.log2(max(m.min(), 5e-324)), np.log2(max(m.max(), 5e-324)), ((f > 0) & (f < 2.0 ** -1022)).sum()))
        np.testing.assert_array_equal(np.delete(ref['m'], at, axis=1), np.delete(ref0['m'], at, axis=1))
        plain = ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR)
        got = ctx.trees_grad_rates(child, blen, rates, weights, **FULL)
        lean = ctx.trees_grad_rates(child, blen, rates, weights, prior=PRIOR)
        same_bits([got[0], lean[0]], [plain, plain], "loglik against phylo_trees_loglik_rates")
        shift = e.sum() * np.log(2.0)
        if place == '2^-900':
            assert (m < 2.0 ** -880).all() and (m > 2.0 ** -960).all()
            assert ((f == 0) | (f >= 2.0 ** -1022)).all()                 # every positive category factor is a normal number
            same_bits(got[1:], got0[1:], "2^-900: the unscaled call's bits")
            same_bits([lean[1]], [got0[1]], "2^-900: grad alone")
            np.testing.assert_allclose(got[0], got0[0] - shift, rtol=1e-12, atol=0)
        elif place in EC.IN_RANGE:
            assert (m >= FLOOR).all() and (m <= ROOMY).all()
            if place == 'at-the-floor':
                assert (m.min(axis=0) < 2.0 ** -1019).all()
                assert ((f > 0) & (f < 2.0 ** -1022)).any()               # a category's factor is subnormal beside an m in range
            assert all(np.isfinite(a).all() for a in got + lean)
            np.testing.assert_allclose(got[0], got0[0] - shift, rtol=1e-12, atol=0)
            close_all(place + " against the restatement on the scaled alignment", got, ref)
            close(place + " grad against the unscaled call", got[1], got0[1], ref0['scale'])
            close(place + " curv against the unscaled call", got[2], got0[2], ref0['scale'])
            close(place + " grad alone against the unscaled call", lean[1], got0[1], ref0['scale'])
            ex_r, ex_w = GC.floor_excess(m, blen, weights)
            GC.close_with_excess(place + " drate against the unscaled call", got[3], got0[3], ref0['drate_scale'], ex_r)
            GC.close_with_excess(place + " dweight against the unscaled call", got[4], got0[4], ref0['dweight'], ex_w)
        else:
            assert (m < FLOOR).all() and all_nan([ref[k] for k in ('grad', 'curv', 'drate', 'dweight')])
            if place == 'just-below':
                assert (m.max(axis=0) >= 2.0 ** -1021).all()
            if place == 'zero':
                assert (m == 0).all() and (got[0] == -np.inf).all()
            else:
                assert (m > 0).all() and np.isfinite(got[0]).all()
            assert all_nan(got[1:]) and all_nan(lean[1:])


def test_one_site_below_the_floor_spoils_its_tree_alone():
    """a set in which only SOME trees see a site value below the floor: the others keep what they have without it -- grad and
    curv within TOL_RATES; drate and dweight within the near-floor bound, because the site value of those trees at the scaled
    site lies just above the floor and a category's factor beside it is subnormal (the restatement alone, scaled against
    unscaled, is 763 units of plain TOL_RATES' scale away in drate: test_treegrad_edges_cpu.py)"""
    g, child, blen, Q, got0, ref0 = unscaled('I+G4')
    rates, weights = MIX_I_G4
    gs = GC.scale_one_site(g, GC.one_site_below(ref0['m']))
    with make_ctx(gs, Q, pi=PRIOR, tile=64) as ctx:
        with GC.hardware_fma():
            ref = reference(ctx, child, blen, Q, PRIOR, gs, rates, weights)
        out = (ref['m'] < FLOOR).any(axis=1)
        assert 1 <= out.sum() < out.size and (ref['m'] > 0).all(), ref['m'][:, 129]
        ex_r, ex_w = GC.floor_excess(ref['m'][~out][:, [129]], blen[~out], weights)
        for k in ('grad', 'curv', 'drate', 'dweight'):                    # the restatement first
            assert np.isnan(ref[k][out]).all()
        close("restatement, in-range trees, grad", ref['grad'][~out], ref0['grad'][~out], ref0['scale'][~out])
        close("restatement, in-range trees, curv", ref['curv'][~out], ref0['curv'][~out], ref0['scale'][~out])
        GC.close_with_excess("restatement, in-range trees, drate", ref['drate'][~out], ref0['drate'][~out], ref0['drate_scale'][~out], ex_r)
        GC.close_with_excess("restatement, in-range trees, dweight", ref['dweight'][~out], ref0['dweight'][~out], ref0['dweight'][~out], ex_w)
        got = ctx.trees_grad_rates(child, blen, rates, weights, **FULL)
        same_bits([got[0]], [ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR)], "loglik")
        assert np.isfinite(got[0]).all()
        assert all_nan([a[out] for a in got[1:]])
        close("in-range trees, grad", got[1][~out], got0[1][~out], ref0['scale'][~out])
        close("in-range trees, curv", got[2][~out], got0[2][~out], ref0['scale'][~out])
        GC.close_with_excess("in-range trees, drate", got[3][~out], got0[3][~out], ref0['drate_scale'][~out], ex_r)
        GC.close_with_excess("in-range trees, dweight", got[4][~out], got0[4][~out], ref0['dweight'][~out], ex_w)
