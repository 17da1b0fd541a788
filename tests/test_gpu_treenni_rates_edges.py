"""phylo_trees_nni_rates on the device where test_gpu_treenni_rates.py stops (inputs:
treenni_rates_edges_cases.py, treegrad_edges_cases.py, trees_edges_cases.py).  A: items of one to five strips under the default
site tile, so that acc is carried from strip to strip and every plane of the node store is written again over the outer partials
the previous strip left.  B: 129 to 512 taxa under genuine mixtures -- five and sixteen DIFFERENT planes, so that a partial or an
outer partial read from or left in the wrong plane shows, with impossible neighbours and missing root moves in deep trees; two
strips at 257 taxa; per-tree mixtures at depth.  C: a workgroup's second 512-taxon item under the C-dependent cap of the grid (25
workgroups under +I+G4, 8 under sixteen categories), on C planes full of outer partials and an acc of 1022 entries to clear.
D: the mixed site value m near the floor of the double range: below 2^-1020 every entry of the tree is NaN beside
phylo_trees_loglik_rates' loglik bits; at and above it delta is the unscaled alignment's within plain TOL_NNI_RATES (no allowance:
treenni_rates_edges_cases.py says why), and random columns over 390 and 400 taxa reach that floor by themselves.

ptnr_updown is a kernel of its own; what test_gpu_treenni_edges.py shows of ptn_updown says nothing about it.  delta is held to
the restatement (treenni_rates_ref.py on the device's own matrices of every category) within TOL_NNI_RATES, above 128 taxa within
TOL_NNI_RATES_BIG, and loglik + delta to phylo_trees_loglik_rates of explicitly built neighbours within TOL_EXPL_RATES(_BIG), all
measured at 50 digits on the CPU (test_treenni_rates_edges_cpu.py) before the kernel ran here.  Every test asserts its
preconditions from the restatement before it compares anything, prints the worst ratio to its bound, and holds loglik to
phylo_trees_loglik_rates' bits."""
import functools

import numpy as np
import pytest

import treegrad_edges_cases as GC
import treegrad_ref as TR
import treenni_cases as NC
import treenni_rates_edges_cases as XC
import trees_edges_cases as EC
from test_gpu_treenni_rates import close, device_matrices, explicit, missing_moves, same_bits
from test_gpu_trees_edges import compute_units
from test_gpu_trees_loglik import alignment, bits, gtr_Q, make_ctx, random_trees
from treegrad_rates_cases import MIX_I_G4
from treenni_rates_edges_cases import TOL_EXPL_RATES_BIG, TOL_NNI_RATES_BIG
from trees_edges_cases import FLOOR, PRIOR, ROOMY

pytestmark = pytest.mark.gpu


def restated(ctx, child, blen, g, rates, weights):
    """the restatement on the device's own matrices of every category, with the site values: loglik, delta, absd, m"""
    return XC.restated(child, device_matrices(ctx, blen, rates), PRIOR, g, rates, weights)


def call(ctx, child, blen, rates, weights):
    """phylo_trees_nni_rates (whose stats ctx.last_trees_stats then holds), its loglik held to phylo_trees_loglik_rates' bits"""
    want = ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR)
    ll, delta = ctx.trees_nni_rates(child, blen, rates, weights, prior=PRIOR)
    same_bits([ll], [want], "loglik against phylo_trees_loglik_rates")
    assert delta.shape == blen.shape
    return ll, delta


def repeat_and_reverse(ctx, child, blen, rates, weights, got, what):
    same_bits(ctx.trees_nni_rates(child, blen, rates, weights, prior=PRIOR), got, what + ": a repeated call")
    rev = ctx.trees_nni_rates(child[::-1], blen[::-1], rates, weights, prior=PRIOR)
    same_bits([a[::-1] for a in rev], got, what + ": the set reversed")


# ---- A. one item of several strips ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GC.STRIPS))
def test_strips(name, monkeypatch):
    kw = GC.STRIPS[name]
    N, S = kw['N'], kw['S']
    rates, weights = GC.MIXTURES[kw['mix']]
    g = alignment(N, S, 100 + N + S, kw.get('gaps', False), kw.get('generic', False))
    Q = gtr_Q()
    child, blen = random_trees(N, 5, XC.T_STRIPS)
    assert child.shape[0] == 7 and (blen == 0).any()                      # trees with zero-length branches
    per_chunk = 4 if kw.get('generic') else 5                             # coded leaves: the gap rows too
    miss = missing_moves(child)
    what = "%s (%d strips)" % (name, -(-S // 128))
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        assert ctx.site_tile() >= S                                       # the default tile: one item of ceil(S / 128) strips
        rll, rdelta, absd, m = restated(ctx, child, blen, g, rates, weights)
        assert np.isfinite(rll).all() and (m > 2.0 ** -200).all()         # the preconditions, before anything is compared
        np.testing.assert_array_equal(np.isnan(rdelta), miss)
        ll, delta = call(ctx, child, blen, rates, weights)
        st = ctx.last_trees_stats
        assert st['n_launches'] == per_chunk and st['units'] == 7 * S * (N - 1) * rates.size
        np.testing.assert_allclose(ll, rll, rtol=1e-12, atol=0)
        np.testing.assert_array_equal(np.isnan(delta), miss, err_msg="NaN exactly where a move does not exist")
        close(what, delta, rdelta, absd, S)                               # -inf exactly where the restatement has it
        explicit(what, ctx, child[:3], blen[:3], ll, delta, PRIOR, S, rates, weights)
        repeat_and_reverse(ctx, child, blen, rates, weights, (ll, delta), what)
    monkeypatch.setenv('PHYLO_TREES_CHUNK', '2')                          # read when the context is created
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        same_bits(ctx.trees_nni_rates(child, blen, rates, weights, prior=PRIOR), (ll, delta), what + ": chunks of 2")
        assert ctx.last_trees_stats['n_launches'] == 4 * per_chunk
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:                        # ceil(S / 64) items of one strip each: another order of the sum,
        assert ctx.site_tile() == 64                                      # so within the tolerance and no bits (test_two_strips_per_tile)
        ll64, delta64 = call(ctx, child, blen, rates, weights)
        np.testing.assert_allclose(ll64, ll, rtol=1e-12, atol=0)
        close(what + ", tile 64 against the restatement", delta64, rdelta, absd, S)
        close(what + ", strips against tile 64", delta, delta64, absd, S)


# ---- B. 129 to 512 taxa under genuine mixtures -----------------------------------------------------------------------------------------
def many_taxa(name, mix, sample, chunks, monkeypatch):
    kw = EC.BIG[name]
    N, S, tile = kw['N'], kw['S'], kw.get('tile')
    per_chunk = 4 if kw.get('generic') else 5
    g, child, blen, Q = EC.big_case(name)
    n = child.shape[0]
    rates, weights = mix
    what = "%s C%d" % (name, rates.size)
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR, tile=tile) as ctx:
        assert -(-S // ctx.site_tile()) == (3 if tile else 1)
        M = device_matrices(ctx, blen[sample], rates)
        rll, rdelta, absd, m = XC.restated(child[sample], M, PRIOR, g, rates, weights, exact_mix=N < 512)
        miss = missing_moves(child)
        print("%s: reference site values in [2^%.1f, 2^%.1f], %d -inf, %d NaN" % (what, np.log2(m.min()), np.log2(m.max()), np.isneginf(rdelta).sum(), miss.sum()))
        assert (m >= ROOMY).all() and np.isfinite(m).all()                # the preconditions, before anything is compared
        np.testing.assert_array_equal(np.isnan(rdelta), miss[sample])
        if kw['shape'] == 'balanced':
            assert not np.isneginf(rdelta).any() and not miss.any()
        elif kw['shape'] == 'caterpillar':
            assert np.isneginf(rdelta).any()                              # impossible neighbours: zero-length right-hand branches
            assert miss[:, -1].all()                                      # a leaf at the root: no move across it
        f0 = TR.site_factors(child[sample[0]], M[0, 0], PRIOR, g)         # the invariant class: f_0 = 0 exactly at the variable sites
        direct = (PRIOR * g.prod(axis=0)).sum(axis=-1)
        assert rates[0] == 0.0 and (f0 == 0).any()
        np.testing.assert_array_equal(f0 == 0, direct == 0)
        _, cats = ctx.trees_loglik_rates(child[sample[:1]], blen[sample[:1]], rates, weights, prior=PRIOR, want_cats=True)
        np.testing.assert_array_equal(cats[0, 0] == 0, f0 == 0)           # ... on the device too
        ll, delta = call(ctx, child, blen, rates, weights)
        st = ctx.last_trees_stats
        assert st['units'] == n * S * (N - 1) * rates.size and st['n_launches'] == per_chunk
        assert np.isfinite(ll).all()
        np.testing.assert_allclose(ll[sample], rll, rtol=1e-12, atol=0)
        np.testing.assert_array_equal(np.isnan(delta), miss, err_msg="NaN exactly where a move does not exist")
        close(what, delta[sample], rdelta, absd, S, tol=TOL_NNI_RATES_BIG)        # -inf exactly where the restatement has it
        repeat_and_reverse(ctx, child, blen, rates, weights, (ll, delta), what)
        explicit(what, ctx, child[sample], blen[sample], ll[sample], delta[sample], PRIOR, S, rates, weights, tol=TOL_EXPL_RATES_BIG,
                 moves=NC.move_sample)
    if chunks:
        monkeypatch.setenv('PHYLO_TREES_CHUNK', '2')                      # read when the context is created
        with make_ctx(g, Q, pi=PRIOR, tile=tile) as ctx:
            same_bits(ctx.trees_nni_rates(child, blen, rates, weights, prior=PRIOR), (ll, delta), what + ": chunks of 2")
            assert ctx.last_trees_stats['n_launches'] == 3 * per_chunk


@pytest.mark.parametrize("name", list(EC.BIG))
def test_many_taxa(name, monkeypatch):
    """every shape at 129, 257 and 512 taxa under +I+G4, all five trees: five different planes of the node store"""
    many_taxa(name, MIX_I_G4, list(range(5)), True, monkeypatch)


@pytest.mark.parametrize("name", ['caterpillar-N512', 'generic-balanced-N512'])
def test_512_taxa_16_categories(name, monkeypatch):
    """the real sixteen-category mixture (+I+G15, every weight positive, sixteen different rates): sixteen different planes, 44 KiB
    of LDS, 32 MiB of node store per workgroup.  Trees 0 and 2 against the restatement."""
    assert GC.C16[0].size == 16 and len(set(GC.C16[0].tolist())) == 16 and (GC.C16[1] > 0).all()
    many_taxa(name, GC.C16, [0, 2], False, monkeypatch)


def test_two_strips_at_257_taxa(monkeypatch):
    """257 taxa, S = 200 under a site tile of 256 and +I+G4: ONE item whose strip loop runs at base 0 and 128 over the same five
    planes.  Against the restatement; against tile = 64 within the tolerance only (the order of the sum over sites differs)."""
    g, child, blen, Q = EC.two_strip_case()
    S = g.shape[1]
    rates, weights = MIX_I_G4
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR, tile=256) as ctx:
        assert ctx.site_tile() == 256 and -(-S // ctx.site_tile()) == 1 and 128 < S < 256
        rll, rdelta, absd, m = restated(ctx, child, blen, g, rates, weights)
        assert (m >= ROOMY).all() and np.isfinite(m).all() and not np.isnan(rdelta).any()
        ll, delta = call(ctx, child, blen, rates, weights)
        assert ctx.last_trees_stats['n_launches'] == 5
        np.testing.assert_allclose(ll, rll, rtol=1e-12, atol=0)
        close("two strips", delta, rdelta, absd, S, tol=TOL_NNI_RATES_BIG)
        repeat_and_reverse(ctx, child, blen, rates, weights, (ll, delta), "two strips")
        explicit("two strips", ctx, child, blen, ll, delta, PRIOR, S, rates, weights, tol=TOL_EXPL_RATES_BIG, moves=NC.move_sample)
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        assert -(-S // ctx.site_tile()) == 4
        ll64, delta64 = call(ctx, child, blen, rates, weights)
        np.testing.assert_allclose(ll64, ll, rtol=1e-12, atol=0)
        close("tile 64 against the restatement", delta64, rdelta, absd, S, tol=TOL_NNI_RATES_BIG)
        close("two strips against tile 64", delta, delta64, absd, S, tol=TOL_NNI_RATES_BIG)


def test_per_tree_mixtures_at_depth():
    """random-N257 under five different +I+G4 mixtures: tree t under its own mixture has the bits of the shared call with mixture
    t -- w and P indexed by tree at R = 256"""
    g, child, blen, Q = EC.big_case('random-N257')
    rt, wt = XC.per_tree_mixtures()
    assert rt.shape == (5, 5) and len({r.tobytes() for r in rt}) == 5
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        own = ctx.trees_nni_rates(child, blen, rt, wt, prior=PRIOR)
        assert np.isfinite(own[0]).all() and ctx.last_trees_stats['n_launches'] == 5
        for t in range(5):                                                # phylo_trees_loglik_rates takes one mixture a call
            same_bits([own[0][t:t + 1]], [ctx.trees_loglik_rates(child[t:t + 1], blen[t:t + 1], rt[t], wt[t], prior=PRIOR)], "loglik of tree %d" % t)
        np.testing.assert_array_equal(np.isnan(own[1]), missing_moves(child))
        shared = []
        for t in range(5):
            one = ctx.trees_nni_rates(child, blen, rt[t], wt[t], prior=PRIOR)
            same_bits((own[0][t], own[1][t]), (one[0][t], one[1][t]), "tree %d under its own mixture" % t)
            shared.append(one)
        for t in range(1, 5):                                             # the mixtures do differ in what they give
            assert not np.array_equal(bits(shared[t][1][t]), bits(shared[0][1][t]))
        rll, rdelta, absd, m = XC.restated(child[3:4], device_matrices(ctx, blen[3:4], rt[3]), PRIOR, g, rt[3], wt[3])
        assert (m >= ROOMY).all()
        close("tree 3 under its own mixture", own[1][3:4], rdelta, absd, g.shape[1], tol=TOL_NNI_RATES_BIG)


# ---- C. a workgroup's second item at 512 taxa -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [5, 16])
def test_second_items_512_taxa(C, monkeypatch):
    """more trees of 512 taxa in ONE chunk than the node stores allow workgroups (28 on 25 under +I+G4, 11 on 8 under sixteen
    categories): workgroups 0, 1, 2 take a second tree, of another topology and row order, on C planes that their first item's
    downward pass left full of outer partials and an acc of 1022 entries; against the same trees one item per workgroup, bit for bit"""
    rates, weights = {5: MIX_I_G4, 16: GC.C16}[C]
    cus = compute_units()
    cap = XC.rates_cap(512, C, cus)
    assert rates.size == C and cap == {5: 25, 16: 8}[C]                   # ptnr_make_plan's grid: test_treenni_rates_edges_cpu.py
    T = XC.T_SECOND[C]
    sample = XC.SAMPLE_SECOND[C]
    g, child, blen, Q = EC.large_strided(True, T)
    S = g.shape[1]
    assert T == cap + 3 and sample[-3:] == list(range(cap, T))
    for w in range(cap, T):                                               # one workgroup's two items differ in topology
        assert child[w].tobytes() != child[w - cap].tobytes()
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        assert -(-S // ctx.site_tile()) == 1
        rll, rdelta, absd, m = XC.restated(child[sample], device_matrices(ctx, blen[sample], rates), PRIOR, g, rates, weights, exact_mix=False)
        assert (m >= ROOMY).all() and np.isfinite(m).all()
        np.testing.assert_array_equal(np.isnan(rdelta), missing_moves(child[sample]))
        full = call(ctx, child, blen, rates, weights)
        st = ctx.last_trees_stats
        assert st['n_launches'] == 5 and st['units'] == T * S * 511 * C   # one chunk: T items on `cap` workgroups
        assert np.isfinite(full[0]).all()
        np.testing.assert_array_equal(np.isnan(full[1]), missing_moves(child))
        np.testing.assert_allclose(full[0][sample], rll, rtol=1e-12, atol=0)
        close("N512 C%d, %d items on %d workgroups" % (C, T, cap), full[1][sample], rdelta, absd, S, tol=TOL_NNI_RATES_BIG)
    monkeypatch.setenv('PHYLO_TREES_CHUNK', str(cap))
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        parts = ctx.trees_nni_rates(child, blen, rates, weights, prior=PRIOR)
        assert ctx.last_trees_stats['n_launches'] == 2 * 5
    same_bits(full, parts, "N512 C%d: second items against one item per workgroup" % C)


# ---- D. the floor of the range, on the mixed site value m ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unscaled(mix):
    g, child, blen, Q = EC.scaled_base()
    rates, weights = XC.FLOOR_MIXES[mix]
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        assert ctx.site_tile() == 64
        ll, delta = call(ctx, child, blen, rates, weights)
        rll, rdelta, absd, m = restated(ctx, child, blen, g, rates, weights)
    assert np.isfinite(ll).all() and (m > 2.0 ** -200).all()
    close("unscaled " + mix, delta, rdelta, absd, g.shape[1])             # twelve taxa: the bound of the small trees
    for a in (ll, delta, absd, m):
        a.setflags(write=False)
    return g, child, blen, Q, ll, delta, absd, m


@pytest.mark.parametrize("place,mix", XC.FLOOR_RUNS)
def test_scaled_sites(place, mix):
    g, child, blen, Q, ll0, delta0, absd0, m0 = unscaled(mix)
    rates, weights = XC.FLOOR_MIXES[mix]
    S = g.shape[1]
    e = EC.scaled_exponents(place, m0)                                    # m in place of L: the rule is on the mixture value
    gs = EC.scaled_leaves(g, e)
    at = list(EC.SCALED_SITES)
    miss = missing_moves(child)
    with make_ctx(gs, Q, pi=PRIOR, tile=64) as ctx:
        M = device_matrices(ctx, blen, rates)
        with GC.hardware_fma():                                           # the emulated fma is not the device's below 1e-290
            rll, rdelta, absd, m = XC.restated(child, M, PRIOR, gs, rates, weights)
            fp = np.array([v[:, at] for c, mm in zip(child, M) for v in XC.tree_values(c, mm, PRIOR, gs, weights)[3].values()])
        ms = m[:, at]
        sub = int(((fp > 0) & (fp < 2.0 ** -1022)).sum())
        print(place, mix, "reference: scaled site values in [2^%.1f, 2^%.1f], %d subnormal category factors of neighbours"
              % (np.log2(max(ms.min(), 5e-324)), np.log2(max(ms.max(), 5e-324)), sub))
        np.testing.assert_array_equal(bits(np.delete(m, at, axis=1)), bits(np.delete(m0, at, axis=1)))    # the untouched sites
        ll, delta = call(ctx, child, blen, rates, weights)
        if place in EC.IN_RANGE:
            assert (ms >= FLOOR).all() and (ms <= (2.0 ** -880 if place == '2^-900' else ROOMY)).all() and np.isfinite(ll).all()
            np.testing.assert_array_equal(np.isnan(rdelta), miss)
            np.testing.assert_array_equal(np.isneginf(rdelta), np.isneginf(delta0))
            np.testing.assert_allclose(ll, ll0 - e.sum() * np.log(2.0), rtol=1e-12, atol=0)
            if place == '2^-900':
                assert sub == 0 and ((fp == 0) | (fp >= 2.0 ** -1022)).all()      # every positive category factor is a normal number
                same_bits([delta], [delta0], "2^-900: delta against the unscaled call")
            else:
                if place == 'at-the-floor':
                    assert (ms.min(axis=0) < 2.0 ** -1019).all() and sub >= 1     # subnormal factors beside an m in range
                # the contract near the floor: plain TOL_NNI_RATES, no allowance (treenni_rates_edges_cases.py)
                close(place + " " + mix + " against the restatement on the scaled alignment", delta, rdelta, absd, S)
                close(place + " " + mix + " against the unscaled call", delta, delta0, absd0, S)
                same = bits(delta) == bits(delta0)
                print(place, mix, "%d of %d entries keep the unscaled call's bits" % (same.sum(), same.size))
        else:
            assert (ms < FLOOR).all() and np.isnan(rdelta).all()
            if place == 'just-below':
                assert (ms.max(axis=0) >= 2.0 ** -1021).all()
            if place == 'zero':
                assert (ms == 0).all() and (ll == -np.inf).all()
            else:
                assert (ms > 0).all() and np.isfinite(ll).all()
            assert np.isnan(delta).all()


# ---- D. coded leaves: random columns over 390 and 400 taxa ----------------------------------------------------------------------------
def random_columns(N):
    g, child, blen, Q = EC.random_columns(N)
    rates, weights = MIX_I_G4
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        with GC.hardware_fma():
            rll, rdelta, absd, m = restated(ctx, child, blen, g, rates, weights)
        out = (m < FLOOR).any(axis=1)
        print("N = %d: smallest site value per tree 2^%s, values below the floor %s, loglik %s" % (N, np.log2(m.min(axis=1)).round(1), (m < FLOOR).sum(axis=1), rll))
        assert (m > 0).all() and np.isfinite(rll).all() and np.isnan(rdelta[out]).all()
        ll, delta = call(ctx, child, blen, rates, weights)
        assert np.isfinite(ll).all() and np.isnan(delta[out]).all()
        np.testing.assert_allclose(ll, rll, rtol=1e-12, atol=0)
        return out, m, delta, rdelta, absd, child, g.shape[1]


def test_390_taxa_random_columns_spoil_one_tree():
    """the last N of 300, 310, ... at which tree 0 stays in range under +I+G4: its smallest m is 2^-1015.5, beside subnormal category
    factors; tree 2 has two values below the floor and is NaN in every entry, trees 0 and 1 keep theirs"""
    out, m, delta, rdelta, absd, child, S = random_columns(XC.N_COLUMNS_IN)
    assert out.tolist() == [False, False, True] and m[0].min() < ROOMY
    np.testing.assert_array_equal(np.isnan(delta[~out]), missing_moves(child[~out]))
    close("N390 in-range trees", delta[~out], rdelta[~out], absd[~out], S, tol=TOL_NNI_RATES_BIG)


def test_400_taxa_random_columns_leave_the_range():
    """every tree has site values below the floor, none zero, and a finite loglik: NaN in every entry"""
    out, m, delta, rdelta, absd, child, S = random_columns(XC.N_COLUMNS_OUT)
    assert out.all() and np.isnan(delta).all()
