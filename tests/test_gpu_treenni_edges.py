"""phylo_trees_nni on the device where test_gpu_treenni.py stops (inputs: trees_edges_cases.py).
A: 129 to 512 taxa -- acc[2 (N-1)] behind a stack of 7 to 9 slots, 16 trips of the loops that clear and copy it, ptn_nni_ops
indices up to 510 operations back, impossible neighbours and missing root moves in deep trees; two strips of 128 sites in one
tile at 257 taxa.  B: more work items than ptn_updown has workgroups, so that a workgroup's second item finds the node store its
first item's downward pass left full of outer partials, against the same trees in chunks that fit under the cap.  C: site
factors near the floor of the double range: below 2^-1020 every entry of the tree is NaN beside the loglik bits of
phylo_trees_loglik; at and above it the entries are those of the unscaled alignment.

delta is held to the restatement (treenni_ref.py on the device's own matrices) within TOL_NNI_BIG and loglik + delta to
phylo_trees_loglik of explicitly built neighbours within TOL_EXPL_BIG, both measured at 50 digits on the CPU
(test_treenni_edges_cpu.py) before the kernel ran here.  Every precondition is asserted from the restatement before anything is
compared; every test prints the worst ratio to its bound."""
import numpy as np
import pytest

import treenni_cases as NC
import treenni_ref as NR
import trees_edges_cases as EC
from test_gpu_treenni import close, device_matrices, explicit, missing_moves
from test_gpu_trees_edges import compute_units
from test_gpu_trees_loglik import bits, make_ctx
from treenni_cases import PRIOR, TOL_EXPL_BIG, TOL_NNI_BIG
from trees_edges_cases import FLOOR, ROOMY

pytestmark = pytest.mark.gpu


def restated(ctx, child, blen, g):
    """test_gpu_treenni.reference's restatement on the device's own matrices, with the site factors: loglik, delta, absd, L"""
    res = [NR.tree_nni(c, m, PRIOR, g, want_sites=True) for c, m in zip(child, device_matrices(ctx, blen))]
    return tuple(np.array([r[k] for r in res]) for k in range(4))


def same_bits(got, want, what):
    for name, a, b in zip(('loglik', 'delta'), got, want):
        np.testing.assert_array_equal(bits(a), bits(b), err_msg="%s: %s" % (what, name))


# ---- A. 129 to 512 taxa --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.BIG))
def test_many_taxa(name, monkeypatch):
    kw = EC.BIG[name]
    N, S, tile = kw['N'], kw['S'], kw.get('tile')
    per_chunk = 4 if kw.get('generic') else 5                             # coded leaves: the gap rows too
    g, child, blen, Q = EC.big_case(name)
    n = child.shape[0]
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR, tile=tile) as ctx:
        assert -(-S // ctx.site_tile()) == (3 if tile else 1)
        rll, rdelta, absd, L = restated(ctx, child, blen, g)
        miss = missing_moves(child)
        print("%s: reference site factors in [%.3g, %.3g], %d -inf, %d NaN" % (name, L.min(), L.max(), np.isneginf(rdelta).sum(), miss.sum()))
        assert (L >= ROOMY).all() and np.isfinite(L).all()                # the preconditions, before anything is compared
        np.testing.assert_array_equal(np.isnan(rdelta), miss)
        if kw['shape'] == 'balanced':
            assert not np.isneginf(rdelta).any() and not miss.any()
        elif kw['shape'] == 'caterpillar' or name == 'random-N512':       # (the random trees of 129 and 257 taxa happen to have none)
            assert np.isneginf(rdelta).any()                              # impossible neighbours: zero-length right-hand branches
        if kw['shape'] == 'caterpillar':
            assert miss[:, -1].all()                                      # a leaf at the root: no move across it
        ll, delta = ctx.trees_nni(child, blen, prior=PRIOR)
        st = ctx.last_trees_stats
        assert st['units'] == n * S * (N - 1) and st['n_launches'] == per_chunk
        assert delta.shape == blen.shape and np.isfinite(ll).all()
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)), err_msg="loglik against phylo_trees_loglik")
        np.testing.assert_allclose(ll, rll, rtol=1e-12, atol=0)
        np.testing.assert_array_equal(np.isnan(delta), miss, err_msg="NaN exactly where a move does not exist")
        close(name, delta, rdelta, absd, S, tol=TOL_NNI_BIG)              # -inf exactly where the restatement has it
        same_bits(ctx.trees_nni(child, blen, prior=PRIOR), (ll, delta), "a repeat call")
        rev = ctx.trees_nni(child[::-1], blen[::-1], prior=PRIOR)         # a tree's bits do not depend on its place
        same_bits([a[::-1] for a in rev], (ll, delta), "the trees in reverse order")
        explicit(name, ctx, child, blen, ll, delta, PRIOR, S, tol=TOL_EXPL_BIG, moves=NC.move_sample)
    monkeypatch.setenv('PHYLO_TREES_CHUNK', '2')                          # read when the context is created
    with make_ctx(g, Q, pi=PRIOR, tile=tile) as ctx:
        same_bits(ctx.trees_nni(child, blen, prior=PRIOR), (ll, delta), "chunks of 2")
        assert ctx.last_trees_stats['n_launches'] == 3 * per_chunk


def test_two_strips_per_tile(monkeypatch):
    """257 taxa, S = 200 under a site tile of 256: ONE tile whose strip loop runs at base 0 and 128 over the same node store, 72
    live sites in the second strip.  Against the restatement; against tile = 64 (four tiles, one strip each) loglik and delta
    within their tolerances only: the order of the sum over sites differs between tiles, so no bits are claimed."""
    g, child, blen, Q = EC.two_strip_case()
    S = g.shape[1]
    assert S == 200
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR, tile=256) as ctx:
        assert ctx.site_tile() == 256 and -(-S // ctx.site_tile()) == 1 and 128 < S < 256
        rll, rdelta, absd, L = restated(ctx, child, blen, g)
        assert (L >= ROOMY).all() and np.isfinite(L).all() and not np.isnan(rdelta).any()
        ll, delta = ctx.trees_nni(child, blen, prior=PRIOR)
        assert ctx.last_trees_stats['n_launches'] == 5
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)), err_msg="loglik against phylo_trees_loglik")
        np.testing.assert_allclose(ll, rll, rtol=1e-12, atol=0)
        close("two strips", delta, rdelta, absd, S, tol=TOL_NNI_BIG)
        same_bits(ctx.trees_nni(child, blen, prior=PRIOR), (ll, delta), "a repeat call")
        explicit("two strips", ctx, child, blen, ll, delta, PRIOR, S, tol=TOL_EXPL_BIG, moves=NC.move_sample)
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        assert -(-S // ctx.site_tile()) == 4
        ll64, delta64 = ctx.trees_nni(child, blen, prior=PRIOR)
        np.testing.assert_array_equal(bits(ll64), bits(ctx.trees_loglik(child, blen, prior=PRIOR)), err_msg="tile 64: loglik against phylo_trees_loglik")
        np.testing.assert_allclose(ll64, ll, rtol=1e-12, atol=0)
        close("tile 64 against the restatement", delta64, rdelta, absd, S, tol=TOL_NNI_BIG)
        close("two strips against tile 64", delta, delta64, absd, S, tol=TOL_NNI_BIG)


# ---- B. a workgroup that takes several items -----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ['same', 'mixed'])
def test_strided_items_512_taxa(which, monkeypatch):
    """131 trees of 512 taxa in ONE chunk over 128 workgroups: workgroups 0, 1, 2 take a second item on a node store whose slots
    their first item's downward pass overwrote with outer partials, and on an acc of 1022 entries they must clear again"""
    # the node store's share of the cap, 256 MiB / (511 2 2 KiB): ptn_make_plan caps its grid by the same store bytes as
    # ptg_make_plan (wg_store = (N-1) PTG_U PTG_SLOT_BYTES against PTG_STORE_BYTES), which is what updown_cap restates
    assert EC.updown_cap(512, compute_units()) == 128
    g, child, blen, Q = EC.large_strided(which == 'mixed')
    S, T = g.shape[1], child.shape[0]
    assert T == 131
    if which == 'mixed':
        for w in range(128, T):                                           # one workgroup's two items differ in topology
            assert child[w].tobytes() != child[w - 128].tobytes()
    sample = [0, 1, 2, 64, 127, 128, 129, 130]                            # the first, the 129th, the last
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        assert -(-S // ctx.site_tile()) == 1
        rll, rdelta, absd, L = restated(ctx, child[sample], blen[sample], g)
        assert (L >= ROOMY).all() and np.isfinite(L).all()
        np.testing.assert_array_equal(np.isnan(rdelta), missing_moves(child[sample]))
        full = ctx.trees_nni(child, blen, prior=PRIOR)
        assert ctx.last_trees_stats['n_launches'] == 5                    # one chunk: 131 items, 128 workgroups
        assert np.isfinite(full[0]).all()
        np.testing.assert_array_equal(bits(full[0]), bits(ctx.trees_loglik(child, blen, prior=PRIOR)))
        np.testing.assert_array_equal(np.isnan(full[1]), missing_moves(child))
        np.testing.assert_allclose(full[0][sample], rll, rtol=1e-12, atol=0)
        close("N512 " + which, full[1][sample], rdelta, absd, S, tol=TOL_NNI_BIG)
    monkeypatch.setenv('PHYLO_TREES_CHUNK', '128')
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        parts = ctx.trees_nni(child, blen, prior=PRIOR)
        assert ctx.last_trees_stats['n_launches'] == 2 * 5
    same_bits(full, parts, "N512 %s: strided against one item per workgroup" % which)


def test_strided_items_five_taxa_mixed(monkeypatch):
    """N = 5, three tiles, 8 CUs + 5 items or more in one chunk, tree t of the topology t mod m: a workgroup's second item is a
    tree of another topology and row order than its first (asserted), against chunks of one item per workgroup bit for bit"""
    cus = compute_units()
    cap = EC.updown_cap(5, cus)
    n = EC.strided_T(5, 3, cus)
    g, child, blen, Q = EC.small_mixed(n, cap)
    S = g.shape[1]
    assert (g.sum(axis=2) == 4).any()                                     # gaps
    for w in range(cap, 3 * n):
        assert child[w // 3].tobytes() != child[(w - cap) // 3].tobytes()
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        assert -(-S // ctx.site_tile()) == 3 and 3 * n >= cap + 5 and (3 * n) % cap != 0
        sample = sorted(set(range(8)) | set(range(cap // 3 - 2, n)))      # ... and every tree of a second item
        rll, rdelta, absd, L = restated(ctx, child[sample], blen[sample], g)
        assert (L >= ROOMY).all()
        full = ctx.trees_nni(child, blen, prior=PRIOR)
        assert ctx.last_trees_stats['n_launches'] == 5                    # one chunk
        np.testing.assert_array_equal(bits(full[0]), bits(ctx.trees_loglik(child, blen, prior=PRIOR)))
        np.testing.assert_array_equal(np.isnan(full[1]), missing_moves(child))
        close("N5 mixed", full[1][sample], rdelta, absd, S)               # five taxa: the bound of the small trees
    chunk = cap // 3
    monkeypatch.setenv('PHYLO_TREES_CHUNK', str(chunk))
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        parts = ctx.trees_nni(child, blen, prior=PRIOR)
        assert ctx.last_trees_stats['n_launches'] == -(-n // chunk) * 5
    same_bits(full, parts, "N5 mixed: strided against one item per workgroup")


# ---- C. the floor of the range: generic leaves scaled by exact powers of two ---------------------------------------------------
@pytest.fixture(scope="module")
def unscaled():
    g, child, blen, Q = EC.scaled_base()
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        assert ctx.site_tile() == 64
        ll, delta = ctx.trees_nni(child, blen, prior=PRIOR)
        rll, rdelta, absd, L = restated(ctx, child, blen, g)
    assert np.isfinite(ll).all() and (L > 2.0 ** -200).all()
    close("unscaled", delta, rdelta, absd, g.shape[1])                    # twelve taxa: the bound of the small trees
    for a in (ll, delta, L):
        a.setflags(write=False)
    return g, child, blen, Q, ll, delta, L


@pytest.mark.parametrize("place", EC.PLACES)
def test_scaled_sites(place, unscaled):
    g, child, blen, Q, ll0, delta0, L0 = unscaled
    e = EC.scaled_exponents(place, L0)
    gs = EC.scaled_leaves(g, e)
    at = list(EC.SCALED_SITES)
    miss = missing_moves(child)
    with make_ctx(gs, Q, pi=PRIOR, tile=64) as ctx:
        rll, rdelta, _, L = restated(ctx, child, blen, gs)
        print(place, "reference: scaled site factors in [%.3g, %.3g]" % (L[:, at].min(), L[:, at].max()))
        np.testing.assert_array_equal(np.delete(L, at, axis=1), np.delete(L0, at, axis=1))
        ll, delta = ctx.trees_nni(child, blen, prior=PRIOR)
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)), err_msg="loglik against phylo_trees_loglik")
        if place in EC.IN_RANGE:
            assert (L[:, at] >= FLOOR).all() and (L[:, at] <= (2.0 ** -880 if place == '2^-900' else ROOMY)).all() and np.isfinite(ll).all()
            np.testing.assert_array_equal(np.isnan(rdelta), miss)
            np.testing.assert_allclose(ll, ll0 - e.sum() * np.log(2.0), rtol=1e-12, atol=0)
            if place == 'at-the-floor':
                # beside a site factor in [2^-1020, 2^-1019) a neighbour's own factor may be subnormal, where neither the device
                # nor the restatement holds 53 bits: the standing of test_gpu_treenni's floor test
                assert (L[:, at].min(axis=0) < 2.0 ** -1019).all()
                np.testing.assert_array_equal(np.isnan(delta), miss)
                np.testing.assert_array_equal(np.isneginf(delta), np.isneginf(delta0))
                fin = np.isfinite(delta0)
                same = bits(delta) == bits(delta0)
                print(place, "%d of %d entries keep the unscaled call's bits, the others move by at most %.3g"
                      % (same.sum(), same.size, np.abs(delta[fin] - delta0[fin]).max()))
                np.testing.assert_allclose(delta[fin], delta0[fin], rtol=1e-6, atol=1e-6)
            else:
                np.testing.assert_array_equal(bits(delta), bits(delta0), err_msg="delta against the unscaled call")
        else:
            assert (L[:, at] < FLOOR).all() and np.isnan(rdelta).all()
            if place == 'just-below':
                assert (L[:, at].max(axis=0) >= 2.0 ** -1021).all()
            if place == 'zero':
                assert (L[:, at] == 0).all() and (ll == -np.inf).all()
            else:
                assert (L[:, at] > 0).all() and np.isfinite(ll).all()
            assert np.isnan(delta).all()


# ---- C. coded leaves: random columns over 300 and 310 taxa -----------------------------------------------------------------------
def test_300_taxa_random_columns_stay_in_range():
    g, child, blen, Q = EC.random_columns(300)
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        rll, rdelta, absd, L = restated(ctx, child, blen, g)
        print("N = 300: smallest site factor per tree", L.min(axis=1))
        assert (L >= FLOOR).all() and L.min() < 1e-300
        np.testing.assert_array_equal(np.isnan(rdelta), missing_moves(child))
        ll, delta = ctx.trees_nni(child, blen, prior=PRIOR)
        assert np.isfinite(ll).all()
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)))
        np.testing.assert_allclose(ll, rll, rtol=1e-12, atol=0)
        close("N300", delta, rdelta, absd, g.shape[1], tol=TOL_NNI_BIG)


def test_310_taxa_random_columns_leave_the_range():
    """Trees with subnormal site factors, none zero, and a finite loglik: NaN in every entry beside phylo_trees_loglik's bits"""
    g, child, blen, Q = EC.random_columns(310)
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        rll, rdelta, absd, L = restated(ctx, child, blen, g)
        out = (L < FLOOR).any(axis=1)
        print("N = 310: smallest site factor per tree", L.min(axis=1), "factors below the floor", (L < FLOOR).sum(axis=1), "loglik", rll)
        assert out.any() and out[0] and np.isfinite(rll[0]) and (L[0] > 0).all() and np.isnan(rdelta[out]).all()
        ll, delta = ctx.trees_nni(child, blen, prior=PRIOR)
        print("device: loglik", ll, "entries not NaN:", (~np.isnan(delta)).sum(axis=(1, 2)))
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PRIOR)))
        assert np.isfinite(ll[0]) and np.isnan(delta[out]).all()
        if (~out).any():                                                  # a tree that stays in range: the reference
            close("N310 in-range", delta[~out], rdelta[~out], absd[~out], g.shape[1], tol=TOL_NNI_BIG)
