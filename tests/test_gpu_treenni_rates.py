"""phylo_trees_nni_rates on the device: the change of the MIXTURE log-likelihood of every tree of a set
under each of its nearest-neighbour interchanges.  loglik is held to phylo_trees_loglik_rates' bits; delta to the NumPy restatement
(treenni_rates_ref.py, fed with the device's own branch matrices of every category) within TOL_NNI_RATES (S + sum_s |d_s| +
|value|), and for N <= 12 loglik + delta to phylo_trees_loglik_rates of the explicitly built neighbour within TOL_EXPL_RATES
(S + sum_s |log m_s| + sum_s |log m'_s|) -- both bounds set from 50-digit arithmetic before the kernel ran
(treenni_rates_cases.py).  Then the bit identities (repeats, place, chunks, per-tree mixtures, the one-rate call), more items than
workgroups, the large corner, the NaN and -inf rules, refusals, what the call leaves alone.

Every test here needs Context.trees_nni_rates: AttributeError without it."""
import ctypes as C

import numpy as np
import pytest

import treenni_cases as NC
import treenni_rates_cases as RC
import treenni_rates_ref as RR
import trees_edges_cases as EC
from oracle import cpu_ref as O
from phylo_amd import _ffi, model
from phylo_amd import rates as R
from phylo_amd import treepost as TP
from phylo_amd.datasets import load_dataset
from phylo_amd.treesearch import apply_nni, nni_moves
from test_gpu_trees_edges import compute_units
from test_gpu_trees_loglik import PI, alignment, bits, gtr_Q, make_ctx, random_trees, shaped_trees
from treegrad_rates_cases import MIX_I_G4
from treegrad_ref import FLOOR
from treenni_rates_cases import PRIOR, TOL_EXPL_RATES, TOL_NNI_RATES
from trees_cases import balanced_rows, caterpillar_rows

pytestmark = pytest.mark.gpu

MODELS = {
    'C1': (np.array([1.3]), np.array([0.9])),
    'C2': R.rate_model(0.5, 2),
    'C3-weight0': (np.array([0.2, 1.0, 2.5]), np.array([0.5, 0.0, 0.5])),
    'C5': MIX_I_G4,                                          # +I+G4: a rate-0 category of weight 0.1
    'C16': R.rate_model(0.7, 15, 0.05),
}


def same_bits(got, want, what):
    for a, b in zip(got, want):
        np.testing.assert_array_equal(bits(a), bits(b), err_msg=what)


def device_matrices(ctx, blen, rates):
    """[T][C][N-1][2][4][4]: ctx.expm_batched of rate * blen (the host's one multiply); rates [C] or [T][C]"""
    rates = np.asarray(rates, dtype=np.float64)
    n = len(blen)
    rt = rates if rates.ndim == 2 else np.broadcast_to(rates, (n, rates.size))
    return np.array([[ctx.expm_batched((rt[t, c] * blen[t]).reshape(-1)).reshape(blen[t].shape + (4, 4)) for c in range(rt.shape[1])]
                     for t in range(n)])


def reference(ctx, child, blen, prior, g, rates, weights):
    """the restatement on the device's own matrices: expm differences stay out of the comparison"""
    return RR.trees_nni_rates(child, device_matrices(ctx, blen, rates), prior, g, rates, weights)


def close(name, got, ref, absd, S, tol=TOL_NNI_RATES):
    """NaN where the restatement has NaN, -inf where it has -inf, elsewhere within tol (S + sum |d_s| + |value|)"""
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=name + ": NaN entries")
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref), err_msg=name + ": -inf entries")
    at = np.isfinite(ref)
    assert np.isfinite(got[at]).all(), name
    err = np.abs(got[at] - ref[at]) / (S + absd[at] + np.abs(ref[at]))
    print("%s: worst |device - restatement| / (S + sum |d_s| + |value|) = %.3g (bound %.3g) over %d entries, %d -inf, %d NaN"
          % (name, err.max() if err.size else 0.0, tol, err.size, np.isneginf(ref).sum(), np.isnan(ref).sum()))
    assert (err <= tol).all(), (name, float(err.max()), tol)


def missing_moves(child):
    out = np.ones(child.shape, dtype=bool)
    for t, c in enumerate(child):
        for mv in nni_moves(c):
            out[t][mv] = False
    return out


def explicit(name, ctx, child, blen, ll, delta, prior, S, rates, weights, tol=TOL_EXPL_RATES, moves=nni_moves):
    """loglik + delta against phylo_trees_loglik_rates of every explicitly built neighbour (moves: which of a tree's moves, every
    one by default; tol: the bound of the deep trees, treenni_rates_edges_cases.TOL_EXPL_RATES_BIG).  Returns the worst ratio to
    the bound."""
    _, sites = ctx.trees_loglik_rates(child, blen, rates, weights, prior=prior, want_sites=True)
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
    ll2, sites2 = ctx.trees_loglik_rates(np.array(cs), np.array(bs), rates, weights, prior=prior, want_sites=True)
    worst = 0.0
    for (t, r, sd), x, s2 in zip(at, ll2, sites2):
        lhs = ll[t] + delta[t, r, sd]
        if np.isneginf(x) or np.isneginf(lhs):
            assert x == lhs, (name, t, r, sd, lhs, x)
            continue
        err = abs(lhs - x) / (S + a0[t] + np.abs(np.log(s2)).sum())
        worst = max(worst, err)
        assert err <= tol, (name, t, r, sd, lhs, x, err, tol)
    print("%s: worst |(loglik + delta) - loglik of the neighbour| / (S + sum |log m| + sum |log m'|) = %.3g (bound %.3g) over %d moves"
          % (name, worst, tol, len(at)))
    return worst / tol


# ---- 1. shapes, conditions and mixtures -------------------------------------------------------------------------------------------
def case(N, S, **kw):
    return dict(N=N, S=S, **kw)


T = 5
CASES = {
    'N5-S1': case(5, 1), 'N5-S63': case(5, 63), 'N12-S65': case(12, 65), 'N12-S129': case(12, 129),
    'three-tiles': case(12, 130, tile=64),
    'N5-caterpillar': case(5, 65, shape=caterpillar_rows), 'N5-balanced': case(5, 65, shape=balanced_rows),
    'N12-caterpillar': case(12, 65, shape=caterpillar_rows), 'N12-balanced': case(12, 65, shape=balanced_rows),
    'generic': case(12, 130, generic=True), 'gaps': case(12, 130, gaps=True), 'jc69': case(12, 130, jc=True),
    'N64-caterpillar': case(64, 65, shape=caterpillar_rows, chunk=2),
}
RUNS = [('N5-S1', 'C5'), ('N5-S1', 'C1'), ('N5-S63', 'C2'), ('N12-S65', 'C5'), ('N12-S65', 'C1'), ('N12-S65', 'C16'), ('N12-S129', 'C3-weight0'),
        ('N12-S129', 'C5'), ('three-tiles', 'C5'), ('three-tiles', 'C2'), ('N5-caterpillar', 'C3-weight0'), ('N5-balanced', 'C16'),
        ('N12-caterpillar', 'C2'), ('N12-balanced', 'C5'), ('generic', 'C5'), ('generic', 'C16'), ('gaps', 'C5'), ('gaps', 'C2'),
        ('jc69', 'C5'), ('N64-caterpillar', 'C2')]


@pytest.mark.parametrize("name,mname", RUNS, ids=['%s-%s' % r for r in RUNS])
def test_against_the_reference(name, mname, monkeypatch):
    kw = CASES[name]
    N, S, jc = kw['N'], kw['S'], kw.get('jc', False)
    rates, weights = MODELS[mname]
    nc = rates.size
    g = alignment(N, S, 100 + N + S, kw.get('gaps', False), kw.get('generic', False))
    Q = O.jc_Q() if jc else gtr_Q()
    child, blen = shaped_trees(kw['shape'], N, 5, T) if 'shape' in kw else random_trees(N, 5, T)
    assert (blen == 0).any()                                              # trees with zero-length branches
    chunk = kw.get('chunk', 3)
    monkeypatch.setenv('PHYLO_TREES_CHUNK', str(chunk))                   # read when the context is created: several chunks
    with make_ctx(g, Q, jc=jc, tile=kw.get('tile')) as ctx:
        if 'tile' in kw:
            assert ctx.site_tile() == 64 and -(-S // 64) == 3
        ll, delta = ctx.trees_nni_rates(child, blen, rates, weights, prior=PRIOR)
        st = ctx.last_trees_stats
        assert st['units'] == T * S * (N - 1) * nc and st['sweep_ms'] > 0
        assert st['n_launches'] == -(-T // chunk) * (4 if kw.get('generic') else 5)      # coded leaves: the gap rows too
        assert delta.shape == blen.shape
        same_bits([ll], [ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR)], "loglik against phylo_trees_loglik_rates")
        assert np.isfinite(ll).all()
        np.testing.assert_array_equal(np.isnan(delta), missing_moves(child), err_msg="NaN exactly where a move does not exist")
        rll, rdelta, absd = reference(ctx, child, blen, PRIOR, g, rates, weights)
        np.testing.assert_allclose(ll, rll, rtol=1e-12, atol=0)
        close("%s %s" % (name, mname), delta, rdelta, absd, S)
        same_bits(ctx.trees_nni_rates(child, blen, rates, weights, prior=PRIOR), (ll, delta), "a repeated call")
        rev = ctx.trees_nni_rates(child[::-1], blen[::-1], rates, weights, prior=PRIOR)
        same_bits((rev[0][::-1], rev[1][::-1]), (ll, delta), "a tree's bits do not depend on its place")
        sub = ctx.trees_nni_rates(child[::2], blen[::2], rates, weights, prior=PRIOR)
        same_bits(sub, (ll[::2], delta[::2]), "a strided subset")
        if N <= 12:
            explicit("%s %s" % (name, mname), ctx, child[:3], blen[:3], ll, delta, PRIOR, S, rates, weights)


def rooted_shapes5():
    """every rooted shape of 5 leaves as rows: a 4-leaf shape and a leaf at the root (either side), a 3-leaf shape and a cherry"""
    out = []
    for c in NC.rooted_shapes(4):
        c = np.where(c >= 4, c + 1, c)                                    # the internal nodes of five leaves start at 5
        out.append(np.vstack([c, [[7, 4]]]).astype(np.int32))
        out.append(np.vstack([c, [[4, 7]]]).astype(np.int32))
    out.append(np.array([[0, 1], [5, 2], [3, 4], [6, 7]], dtype=np.int32))
    out.append(np.array([[3, 4], [0, 1], [6, 2], [5, 7]], dtype=np.int32))
    return out


@pytest.mark.parametrize("N", [4, 5])
@pytest.mark.parametrize("generic", [False, True], ids=['coded', 'generic'])
def test_every_rooted_shape(N, generic):
    """N = 4 and 5: every rooted shape, a root with a leaf child on either side and a root with two internal children included,
    under several labellings, +I+G4"""
    S = 65
    rng = np.random.default_rng(N)
    g = alignment(N, S, 7 + N, gaps=True, generic=generic)
    rates, weights = MIX_I_G4
    child, blen = [], []
    for c in (NC.rooted_shapes(4) if N == 4 else rooted_shapes5()):
        for _ in range(2):
            perm = rng.permutation(N)
            child.append(np.where(c < N, perm[np.minimum(c, N - 1)], c).astype(np.int32))
            blen.append(rng.exponential(0.1, (N - 1, 2)))
    child, blen = np.array(child), np.array(blen)
    with make_ctx(g, gtr_Q()) as ctx:
        ll, delta = ctx.trees_nni_rates(child, blen, rates, weights, prior=PRIOR)
        same_bits([ll], [ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR)], "loglik")
        miss = missing_moves(child)
        assert miss[:, :-1].sum() == 0 and miss[:, -1].any() and not miss[:, -1].all()
        np.testing.assert_array_equal(np.isnan(delta), miss)
        rll, rdelta, absd = reference(ctx, child, blen, PRIOR, g, rates, weights)
        close("N%d shapes" % N, delta, rdelta, absd, S)
        explicit("N%d shapes" % N, ctx, child, blen, ll, delta, PRIOR, S, rates, weights)


# ---- 2. bit identities ------------------------------------------------------------------------------------------------------------
def test_chunks_give_the_same_bits(monkeypatch):
    g = alignment(12, 130, 31, gaps=True)
    child, blen = random_trees(12, 6, 11)
    rates, weights = MIX_I_G4
    got = {}
    for chunk in ('0', '5', '2'):
        monkeypatch.setenv('PHYLO_TREES_CHUNK', chunk)
        with make_ctx(g, gtr_Q(), tile=64) as ctx:
            got[chunk] = ctx.trees_nni_rates(child, blen, rates, weights)
            assert ctx.last_trees_stats['n_launches'] == 5 * {'0': 1, '5': 3, '2': 6}[chunk]
    for chunk in ('5', '2'):
        same_bits(got[chunk], got['0'], "chunks of " + chunk)


def test_per_tree_mixtures():
    """per_tree == 1 with T copies of one mixture gives per_tree == 0's bits; different mixtures per tree give, tree by tree, the
    bits of T shared calls"""
    N, S, n = 12, 130, 6
    g = alignment(N, S, 33, gaps=True)
    child, blen = random_trees(N, 7, n)
    rates, weights = MIX_I_G4
    with make_ctx(g, gtr_Q(), tile=64) as ctx:
        shared = ctx.trees_nni_rates(child, blen, rates, weights, prior=PRIOR)
        same_bits(ctx.trees_nni_rates(child, blen, np.tile(rates, (n, 1)), np.tile(weights, (n, 1)), prior=PRIOR), shared, "T copies")
        mixes = [R.rate_model(a, 4, p, keep_invariant=True) for a, p in zip((0.2, 0.5, 1.0, 2.0, 5.0, 0.7), (0.0, 0.1, 0.2, 0.05, 0.3, 0.0))]
        rt, wt = np.array([m[0] for m in mixes]), np.array([m[1] for m in mixes])
        assert rt.shape == (n, 5)
        own = ctx.trees_nni_rates(child, blen, rt, wt, prior=PRIOR)
        for t in range(n):
            one = ctx.trees_nni_rates(child, blen, rt[t], wt[t], prior=PRIOR)
            same_bits((own[0][t], own[1][t]), (one[0][t], one[1][t]), "tree %d under its own mixture" % t)
        assert not np.array_equal(bits(own[1]), bits(shared[1]))


@pytest.mark.parametrize("generic", [False, True], ids=['coded', 'generic'])
def test_degenerate_mixtures_are_the_one_rate_call(generic):
    """one category of rate 1 and weight 1, and sixteen of which the two at positions 3 and 15 have rate 1 and weight 1/2 and the
    others weight 0: m = f and m' = f' exactly, the contract names the same chains, the build has -ffp-contract=off -- delta is
    phylo_trees_nni's bit for bit"""
    N, S = 12, 130
    g = alignment(N, S, 35, gaps=True, generic=generic)
    child, blen = random_trees(N, 8, 7)
    with make_ctx(g, gtr_Q(), tile=64) as ctx:
        plain = ctx.trees_nni(child, blen, prior=PRIOR)
        assert np.isneginf(plain[1]).any() or (blen == 0).any()
        same_bits(ctx.trees_nni_rates(child, blen, [1.0], [1.0], prior=PRIOR), plain, "C = 1")
        same_bits(ctx.trees_nni_rates(child, blen, *RC.half_half_16(), prior=PRIOR), plain, "1/2, 1/2 at 3 and 15 of 16")


def test_more_items_than_workgroups(monkeypatch):
    """N = 5, three tiles, C = 2: 8 CUs + 5 items or more in ONE chunk (a workgroup takes a second item, a tree of another
    topology) against the same trees in chunks of one item per workgroup, bit for bit: acc and the C planes are clean between items"""
    cus = compute_units()
    cap = EC.updown_cap(5, cus)
    assert cap == 8 * cus                                                 # (two planes of 4 nodes: the store does not cap the grid)
    n = EC.strided_T(5, 3, cus)
    g, child, blen, Q = EC.small_strided(n)
    rates, weights = MODELS['C2']
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        assert 3 * n >= cap + 5 and (3 * n) % cap != 0
        full = ctx.trees_nni_rates(child, blen, rates, weights, prior=PRIOR)
        assert ctx.last_trees_stats['n_launches'] == 5                    # one chunk
        same_bits([full[0]], [ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR)], "loglik")
        sample = sorted(set(range(3)) | set(range(n - 3, n)))             # first items and second items of their workgroups
        _, rdelta, absd = reference(ctx, child[sample], blen[sample], PRIOR, g, rates, weights)
        close("strided", full[1][sample], rdelta, absd, g.shape[1])
    chunk = cap // 3
    monkeypatch.setenv('PHYLO_TREES_CHUNK', str(chunk))
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        parts = ctx.trees_nni_rates(child, blen, rates, weights, prior=PRIOR)
        assert ctx.last_trees_stats['n_launches'] == -(-n // chunk) * 5
    same_bits(parts, full, "one item per workgroup")


def test_large_corner_512_taxa_16_categories():
    """N = 512 under 16 categories, three balanced trees, S = 65: 32 MiB of node store per workgroup (a grid of 3 of the 8 the
    store allows), 44 KiB of LDS.  The mixture is the sixteen-category 1/2, 1/2 one, so delta is held bit for bit to phylo_trees_nni
    (which the edge tests hold to the deep-tree bound); no deep-tree tolerance of its own is asserted here."""
    g, child, blen, Q = EC.large_strided(True, 3)
    assert child.shape == (3, 511, 2) and g.shape[1] == 65 and (256 << 20) // (16 * 511 * 2 * 2048) == 8
    rates, weights = RC.half_half_16()
    with make_ctx(g, Q, pi=PRIOR) as ctx:
        plain = ctx.trees_nni(child, blen, prior=PRIOR)
        got = ctx.trees_nni_rates(child, blen, rates, weights, prior=PRIOR)
        assert np.isfinite(got[0]).all()
        np.testing.assert_array_equal(np.isnan(got[1]), missing_moves(child))
        same_bits(got, plain, "N = 512, C = 16 against phylo_trees_nni")
        same_bits([got[0]], [ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR)], "loglik")


# ---- 3. the NaN and -inf rules ----------------------------------------------------------------------------------------------------
def test_a_dead_site_gives_nan():
    N, S = 5, 70
    g = alignment(N, S, 22, generic=True)
    g[2, 66] = 0.0                                                       # a generic leaf row of zeros kills the site in every tree and category
    child, blen = random_trees(N, 4, 3)
    rates, weights = MIX_I_G4
    with make_ctx(g, gtr_Q()) as ctx:
        ll, delta = ctx.trees_nni_rates(child, blen, rates, weights, prior=PI)
        assert (ll == -np.inf).all() and np.isnan(delta).all()
        same_bits([ll], [ctx.trees_loglik_rates(child, blen, rates, weights, prior=PI)], "loglik")


def test_one_site_below_the_floor_spoils_its_tree_alone():
    """trees_edges_cases' construction on the mixed site value: one site scaled through two generic leaves so that SOME trees see
    m below 2^-1020; those get NaN in every entry beside an unchanged finite loglik, the others keep every entry"""
    g, child, blen, Q = EC.scaled_base()
    rates, weights = MODELS['C2']
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        _, m0 = ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR, want_sites=True)
        _, want = ctx.trees_nni_rates(child, blen, rates, weights, prior=PRIOR)
    s = int(np.argmax(m0.max(axis=0) / m0.min(axis=0)))                   # the site at which the trees differ most ...
    assert m0[:, s].max() > 2 * m0[:, s].min()
    e = int(np.frexp(m0[:, s].max())[1]) + 1019                           # ... its largest value lands in [2^-1020, 2^-1019), its smallest below
    gs = g.copy()
    gs[0, s], gs[1, s] = np.ldexp(g[0, s], -(e // 2)), np.ldexp(g[1, s], -(e - e // 2))
    with make_ctx(gs, Q, pi=PRIOR, tile=64) as ctx:
        ll0, m = ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR, want_sites=True)
        out = (m < FLOOR).any(axis=1)
        assert 1 <= out.sum() < out.size and (m > 0).all(), m[:, s]
        ll, delta = ctx.trees_nni_rates(child, blen, rates, weights, prior=PRIOR)
        same_bits([ll], [ll0], "loglik")
        assert np.isfinite(ll).all() and np.isnan(delta[out]).all()
        np.testing.assert_array_equal(np.isnan(delta[~out]), missing_moves(child[~out]))
        np.testing.assert_allclose(delta[~out], want[~out], rtol=1e-6, atol=1e-6)


def test_impossible_neighbours_need_every_weighted_category():
    """v = (0, 1) with leaf 1 on a zero-length branch, its sibling leaf 2 on a zero-length branch: the move that joins 1 and 2 gives
    every site at which they differ the factor 0 in EVERY category, so -inf under any mixture.  Under +I+G4 a neighbour whose
    invariant class alone has f'_0 = 0 (any variable site) stays finite; with the weight on the invariant class alone it is -inf."""
    N, S = 4, 65
    g = alignment(N, S, 19)
    assert (g[1] != g[2]).any()
    child = np.array([[[0, 1], [4, 2], [5, 3]]] * 2, dtype=np.int32)
    blen = np.array([[[0.1, 0.0], [0.1, 0.0], [0.2, 0.3]], [[0.1, 0.05], [0.1, 0.02], [0.2, 0.3]]])
    rates, weights = MIX_I_G4
    with make_ctx(g, gtr_Q()) as ctx:
        ll, delta = ctx.trees_nni_rates(child, blen, rates, weights, prior=PRIOR)
        rll, rdelta, absd = reference(ctx, child, blen, PRIOR, g, rates, weights)
        assert np.isfinite(ll).all() and rdelta[0, 0, 0] == -np.inf and np.isneginf(rdelta).sum() == 1
        close("zero lengths", delta, rdelta, absd, S)
        explicit("zero lengths", ctx, child, blen, ll, delta, PRIOR, S, rates, weights)
        _, cats = ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR, want_cats=True)
        assert (cats[:, 0] == 0).any()                                    # the invariant class at variable sites: f_0 = 0, all finite above
        # a constant alignment under the invariant class and a slow one: everything finite; the weight on the rate-0 class alone
        # makes every neighbour of a variable alignment impossible -- and the tree itself, so NaN
        w0 = np.array([1.0, 0.0, 0.0, 0.0, 0.0])
        ll2, d2 = ctx.trees_nni_rates(child, blen, rates, w0, prior=PRIOR)
        assert (ll2 == -np.inf).all() and np.isnan(d2).all()
    gc = g.copy()
    gc[:, :] = g[0]                                                       # every column constant: the invariant class explains it
    with make_ctx(gc, gtr_Q()) as ctx:
        ll3, d3 = ctx.trees_nni_rates(child, blen, rates, w0, prior=PRIOR)
        assert np.isfinite(ll3).all() and (np.abs(d3[~np.isnan(d3)]) <= S * 2.0 ** -52).all()   # rate 0: every topology has the same factor (m (1 / m) is 1 to a rounding)


def test_invariant_class_at_variable_sites_is_finite():
    N, S = 8, 130
    g = alignment(N, S, 23)                                              # coded, no gaps: the sites are variable ...
    g[:, ::7] = g[0, ::7]                                                # ... but every seventh, a constant column
    child, blen = random_trees(N, 4, 5)
    blen = blen + 0.01
    rates, weights = MIX_I_G4
    with make_ctx(g, gtr_Q(), tile=64) as ctx:
        ll, delta = ctx.trees_nni_rates(child, blen, rates, weights, prior=PI)
        _, cats = ctx.trees_loglik_rates(child, blen, rates, weights, prior=PI, want_cats=True)
        assert (cats[:, 0] == 0).any() and (cats[:, 0] > 0).any()         # f_0 = 0 at variable sites, > 0 at constant ones
        assert np.isfinite(ll).all() and np.isfinite(delta[~missing_moves(child)]).all()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing():
    N, S = 5, 70
    g = alignment(N, S, 41)
    child, blen = random_trees(N, 8, 4)
    child[2] = np.array([[0, 1], [2, 3], [6, 4], [5, 7]], dtype=np.int32)
    rates, weights = R.rate_model(0.5, 4)
    with _ffi.Context(4, N, S) as ctx:
        with pytest.raises(_ffi.PhyloError) as e:
            ctx.trees_nni_rates(child, blen, rates, weights)
        assert e.value.code == -6                                          # PHYLO_ESTATE: no leaves, no model
        ctx.set_leaves(g)
        with pytest.raises(_ffi.PhyloError) as e:
            ctx.trees_nni_rates(child, blen, rates, weights)
        assert e.value.code == -6                                          # no model
        ctx.set_model(gtr_Q(), PI, np.full(N - 1, 10.0), np.full(N - 1, 10.0))
        ref = ctx.trees_nni_rates(child, blen, rates, weights)

        def refused(call, *what):
            with pytest.raises(_ffi.PhyloError) as e:
                call()
            assert e.value.code == -1, str(e.value)
            for x in what:
                assert x in str(e.value), str(e.value)
            same_bits(ctx.trees_nni_rates(child, blen, rates, weights), ref, "a valid call afterwards")

        c = child.copy(); c[2, 2] = [6, 0]
        refused(lambda: ctx.trees_nni_rates(c, blen, rates, weights), 'tree 2, row 2')
        c2 = child.copy(); c2[2, 3] = [5, -1]
        refused(lambda: ctx.trees_nni_rates(c2, blen, rates, weights), 'tree 2, row 3')
        for v in (np.nan, -1e-9, np.inf):
            b = blen.copy(); b[2, 1, 1] = v
            refused(lambda: ctx.trees_nni_rates(child, b, rates, weights), 'tree 2, row 1')
        refused(lambda: ctx.trees_nni_rates(child, blen, [], []), 'C=0')
        refused(lambda: ctx.trees_nni_rates(child, blen, np.ones(17), np.full(17, 1 / 17)), 'C=17')
        rt, wt = np.tile(rates, (4, 1)), np.tile(weights, (4, 1))
        for v in (-1e-9, np.nan, np.inf, -np.inf):
            r = rates.copy(); r[2] = v
            refused(lambda: ctx.trees_nni_rates(child, blen, r, weights), 'rate', 'category 2')
            w = weights.copy(); w[1] = v
            refused(lambda: ctx.trees_nni_rates(child, blen, rates, w), 'weight', 'category 1')
            r = rt.copy(); r[3, 2] = v                                    # under per_tree the message names the tree
            refused(lambda: ctx.trees_nni_rates(child, blen, r, wt), 'tree 3', 'rate', 'category 2')
            w = wt.copy(); w[1, 0] = v
            refused(lambda: ctx.trees_nni_rates(child, blen, rt, w), 'tree 1', 'weight', 'category 0')
        b = blen.copy(); b[1, 3, 0] = 1e308
        refused(lambda: ctx.trees_nni_rates(child, b, [0.5, 1.0, 10.0], [0.3, 0.3, 0.4]), 'tree 1', 'row 3, category 2')
        ch, bl = np.ascontiguousarray(child, dtype=np.int32), np.ascontiguousarray(blen)
        ll, dl = np.empty(4), np.empty(blen.shape)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        raw = lambda n, *a: ctx._check(ctx._lib.phylo_trees_nni_rates(ctx._h, C.c_int(n), *a))
        full = (p(ch), p(bl), C.c_int(4), p(rates), p(weights), C.c_int(0), None, p(ll), p(dl), None)
        for k in (0, 1, 3, 4, 7, 8):                                      # child, blen, rate, weight, loglik, delta
            args = list(full); args[k] = None
            refused(lambda: raw(4, *args), 'NULL')
        for bad in (2, -1):
            args = list(full); args[5] = C.c_int(bad)
            refused(lambda: raw(4, *args), 'per_tree')
        refused(lambda: raw(0, *full), 'T >= 1')
        refused(lambda: raw(-3, *full), 'T >= 1')
        raw(4, *full)                                                     # prior and perf may be NULL
        same_bits([ll, dl], ref, "the raw call")
        with pytest.raises(ValueError):
            ctx.trees_nni_rates(child, blen, rates, weights[:3])
        with pytest.raises(ValueError):
            ctx.trees_nni_rates(child, blen, rt[:3], wt[:3])
        with pytest.raises(ValueError):
            ctx.trees_nni_rates(child[:, :3], blen[:, :3], rates, weights)


# ---- 5. what the call leaves alone ------------------------------------------------------------------------------------------------
def test_sweep_gradients_and_scores_are_left_alone():
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
        rll, rsites = ctx.trees_loglik_rates(child[:7], blen[:7], rates, weights, want_sites=True)
        rl = ctx.rell(rsites, 50, 3, want_reps=True)
        plain = ctx.trees_nni(child[:7], blen[:7])
        tgr = ctx.trees_grad_rates(child[:7], blen[:7], rates, weights, want_curv=True, want_params=True)
        nll, delta = ctx.trees_nni_rates(child, blen, rates, weights)       # between a sweep and its pending reverse pass
        np.testing.assert_array_equal(np.isnan(delta), missing_moves(child))
        same_bits([nll[:7]], [rll], "loglik")
        grad2 = ctx.sweep_backward()
        again = ctx.sweep_fetch()
        for key in ('log_weights', 'log_likelihood', 'left_branches', 'right_branches'):
            np.testing.assert_array_equal(bits(again[key]), bits(out[key]), err_msg=key)
        np.testing.assert_array_equal(again['ancestors'], out['ancestors'])
        assert bits(again['logZ']) == bits(out['logZ'])
        for key in ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q'):
            np.testing.assert_array_equal(bits(grad2[key]), bits(grad[key]), err_msg=key)
        same_bits(ctx.trees_loglik_rates(child[:7], blen[:7], rates, weights, want_sites=True), (rll, rsites), "section 11b")
        same_bits([ctx.rell(rsites, 50, 3, want_reps=True)['rep_loglik']], [rl['rep_loglik']], "section 12")
        same_bits(ctx.trees_grad_rates(child[:7], blen[:7], rates, weights, want_curv=True, want_params=True), tgr, "section 13b")
        same_bits(ctx.trees_nni(child[:7], blen[:7]), plain, "section 14")
        same_bits(ctx.trees_nni_rates(child, blen, rates, weights), (nll, delta), "the call itself, after the others")
        tab = ctx.tree_summary()                                          # a tree summary made before the call still has its branch pass
        ctx.trees_nni_rates(child[:3], blen[:3], rates, weights)
        tb = ctx.tree_branches(tab)
        assert np.isfinite(tb['leaf_stats']).all()
        third = ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)   # the next sweep's bits
        np.testing.assert_array_equal(bits(third['log_weights']), bits(out['log_weights']))
