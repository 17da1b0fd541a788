"""Every kernel that states the sum over sites, on rows that leave the comfortable range.

The suite's other alignments keep every site likelihood in about [1e-13, 1]: the pair form's fall-backs, pm_log's subnormal
rescale, +inf, NaN and negative factors, the validity selects next to a special value, non-finite tile values and the one-launch
sweep's flag-and-redo path never ran.  Here they do: tests/site_product_cases.py builds leaves scaled by powers of two (and coded
leaves under rates of 1e155) whose node likelihoods walk those classes, replays the columns of the C oracle's node rows to
ASSERT that each class occurred in the case at hand, and every output is compared with the C oracle bit for bit (NaN payloads
aside); finite cases also with mpmath at 60 digits, through the bound of tests/test_site_product_host.py.

The gradient of such a sweep is unspecified (pg_rcp is specified on [2^-1020, 2^1020]) and is not tested here."""
import math

import mpmath as mp
import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import cpu_ref as O
from phylo_amd import _ffi
from tests import site_product_cases as SC
from tests import site_product_ref as R

pytestmark = pytest.mark.gpu
PI = np.full((1, 4), 0.25)
LAZY, EAGER, ONE = _ffi.FLAGS_DEFAULT, _ffi.FLAGS_DEFAULT | _ffi.EAGER_NODES, _ffi.FLAGS_DEFAULT | _ffi.ONE_LAUNCH
FORMS = [(LAZY, "launches, lazy nodes"), (EAGER, "eager nodes"), (ONE, "one launch")]
PAIR_CLASSES = SC.PAIR_CLASSES


def same(a, b):
    """the NaN-aware equality of tests/test_gpu_fullsize.py: every bit, or NaN on both sides"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def check(out, ref, what):
    np.testing.assert_array_equal(out['ancestors'], ref['ancestors'], err_msg=what + ": resampling indices")
    np.testing.assert_array_equal(out['merges'], ref['merges'], err_msg=what + ": merges")
    for key in ('log_likelihood', 'log_weights', 'left_branches', 'right_branches'):
        assert same(out[key], ref[key]), "%s: %s differs" % (what, key)
    assert same(out['logZ'], ref['logZ']), (what, out['logZ'], ref['logZ'])


def classes_of(ref, pi, T, need, what):
    """replay the oracle's node rows; every class in `need` must have occurred"""
    counts = SC.replay(SC.site_likelihoods(ref['nodes'], pi), T)
    print(what, counts)
    for c in need:
        assert counts[c] > 0, "%s: the case never reaches class %r: %r" % (what, c, counts)
    return counts


def sample_nodes(ctx, ref, N, K, what):
    for (r, k) in [(0, 0), (N - 2, K - 1), (N // 2, K // 3), (1, K // 2)]:
        assert same(ctx.sweep_node(r, k), ref['nodes'][r, k]), "%s: node (%d,%d)" % (what, r, k)


def generic_Q():
    return O.get_Q(O.init_y_q())


# ---- the pair update on the device ---------------------------------------------------------------------------------------------

def test_pair_update_device_bits_equal_host_bits():
    """phylo_debug_site_product's kernel against its host body on the triples of tests/test_site_product_host.py (2 * 10^6 random,
    the boundary grid, the steered products): every bit of p', E' and extra' of both forms; every branch counted."""
    gp, g1, g2 = R.boundary_grid()
    sp, s1, s2, _ = R.steered_triples()
    rp, r1, r2 = R.random_triples(2_000_000, seed=20)
    p, x1, x2 = np.concatenate([gp, sp, rp]), np.concatenate([g1, s1, r1]), np.concatenate([g2, s2, r2])
    br = R.branch_of(p, x1, x2)
    for i, name in enumerate(R.BRANCHES):
        assert (br == i).sum() > 0, name
    host = _ffi.debug_site_product(p, x1, x2)
    with _ffi.Context(4, 3, 8) as ctx:
        dev = ctx.site_product_probe(p, x1, x2)
    for form in ('pair', 'each'):
        assert same(dev[form][0], host[form][0]), form + ": p'"
        np.testing.assert_array_equal(dev[form][1], host[form][1], err_msg=form + ": E'")
        assert same(dev[form][2], host[form][2]), form + ": extra'"
    assert same(dev['pair'][0], dev['each'][0]) and same(dev['pair'][2], dev['each'][2])
    np.testing.assert_array_equal(dev['pair'][1], dev['each'][1])


# ---- pk_row_loglik: exact control of every factor ------------------------------------------------------------------------------

def rows_of_section_2(S, rng):
    """[n, S] site likelihoods: the families of the host test and one special factor among ordinary ones at the edges of the layout"""
    m = 1.0 + rng.random(S)
    rows = [np.ldexp(m, rng.integers(-1022, 1022, S)), np.ldexp(m, rng.integers(-530, -504, S)), np.ldexp(m, rng.integers(505, 521, S)),
            np.ldexp(m, rng.integers(-600, 601, S))]
    f = rng.uniform(0.01, 1.0, S)
    sub = rng.random(S) < 0.2
    f[sub] = np.ldexp(m[sub], rng.integers(-1074, -1023, int(sub.sum())))
    rows.append(f)
    n_finite = len(rows)
    for at in sorted({0, S - 1, min(63, S - 1), min(64, S - 1), min(2047, S - 1), min(2048, S - 1)}):
        for v in (0.0, math.inf, math.nan, -1.0, 5e-324):
            f = rng.uniform(0.1, 1.0, S)
            f[at] = v
            rows.append(f)
    if S > 2048:                                           # a -inf tile followed by a +inf tile, and the other way round
        for i, j in ((10, S - 5), (S - 5, 10), (2047, 2048)):
            f = rng.uniform(0.1, 1.0, S)
            f[i], f[j] = 0.0, math.inf
            rows.append(f)
    return np.array(rows), n_finite


@pytest.mark.parametrize("S", [1, 63, 64, 65, 129, 2047, 2048, 2049, 5000])
def test_row_loglik_on_the_rows_of_the_host_test(S):
    """ctx.forest_loglik (pk_row_loglik) with pi = 1/4 and rows (4 f, 0, 0, 0): bit for bit the oracle, and the finite rows within
    the derived bound of the 60-digit sum."""
    rng = np.random.default_rng(S)
    f, n_finite = rows_of_section_2(S, rng)
    core = np.zeros((f.shape[0], 1, S, 4))
    with np.errstate(all='ignore'):
        core[:, 0, :, 0] = 4.0 * f
    rec = np.ones((f.shape[0], 1), dtype=np.int32)
    with _ffi.Context(4, 3, S) as ctx:
        ctx.set_model(generic_Q(), PI, np.full(2, 10.0), np.full(2, 10.0))      # the op takes pi from the model
        assert ctx.site_tile() == CO.site_tile(S) == 2048
        out = ctx.forest_loglik(core, rec)
    ref = CO.forest_loglik(PI, core, rec)
    assert same(out, ref), (S, out, ref)
    assert np.isfinite(out[:n_finite]).all() and not np.isfinite(out[n_finite:]).all()
    assert np.isnan(out).any() and (out == math.inf).any() and (out == -math.inf).any()
    for i in range(n_finite):
        exact, bound = R.row_bound(f[i], 2048)
        err = float(abs(mp.mpf(float(out[i])) - exact))
        print("S=%d row %d: |err| %.3g bound %.3g" % (S, i, err, bound))
        assert err <= bound, (S, i, out[i], err, bound)


# ---- pk_tree_prune ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kinds", [SC.FINITE, SC.SPECIAL], ids=["finite", "special"])
def test_tree_loglik_on_scaled_leaves(kinds):
    """a caterpillar over six scaled leaves: root row and log-likelihood bit for bit the oracle; the finite case against mpmath over
    the site likelihoods of the oracle's root row (the contract's doubles, restated with exact rationals), within the derived bound."""
    N, S = 6, 449
    g = SC.scaled_leaves(N, S, 2048, kinds, seed=11)
    left = np.array([-1] * N + [0, 6, 7, 8, 9], dtype=np.int32)
    right = np.array([-1] * N + [1, 2, 3, 4, 5], dtype=np.int32)
    rng = np.random.default_rng(2)
    bl = np.concatenate([np.zeros(N), rng.exponential(0.1, N - 1)])
    br = np.concatenate([np.zeros(N), rng.exponential(0.1, N - 1)])
    Q = generic_Q()
    with _ffi.Context(4, N, S) as ctx:
        ctx.set_model(Q, PI, np.full(N - 1, 10.0), np.full(N - 1, 10.0))
        ll, root = ctx.tree_loglik(left, right, bl, br, 2 * N - 2, g, PI)
    ll_c, root_c = CO.tree_loglik(Q, PI, left, right, bl, br, 2 * N - 2, g)
    assert same(root, root_c) and same(ll, ll_c), (ll, ll_c)
    x = SC.site_likelihoods(root_c, PI)
    counts = SC.replay(x, 2048)
    print("tree", kinds, counts)
    for c in PAIR_CLASSES + ('last', 'col0', 'col63'):
        assert counts[c] > 0, (c, counts)
    if kinds == SC.FINITE:
        exact, bound = R.row_bound(SC.site_likelihoods_fma(root_c, PI), 2048)
        assert math.isfinite(ll) and abs(mp.mpf(ll) - exact) <= bound, (ll, float(abs(mp.mpf(ll) - exact)), bound)
    else:
        assert math.isnan(ll)


# ---- the sweeps ----------------------------------------------------------------------------------------------------------------------

SWEEP_CASES = SC.SWEEP_CASES


@pytest.mark.parametrize("N,S,T,K,kinds,need", SWEEP_CASES,
                         ids=["S%d-T%d-%s" % (c[1], c[2], {SC.SPECIAL: "special", SC.FINITE: "finite", SC.ALLBAD: "allbad", SC.TILES: "tiles"}[c[4]])
                              for c in SWEEP_CASES])
def test_sweep_forms_on_scaled_generic_leaves(N, S, T, K, kinds, need):
    """pk_rank_merge_nostore (pk_rows_run<false,false>), pk_rank_merge (the wave-0 column pass over likbuf), the one-launch sweep's
    flag and out-of-line redo, pk_tile_epilogue where S > tile: bit for bit the oracle, resampling indices included, while
    log-weights turn -inf and NaN particle by particle."""
    tile = T or 2048
    g = SC.scaled_leaves(N, S, tile, kinds, seed=1)
    Q = generic_Q()
    lam = np.full(N - 1, 10.0)
    ctx = None
    CO.set_site_tile(T)
    try:
        ctx = _ffi.Context(K, N, S)
        ctx.set_site_tile(T)
        assert ctx.site_tile() == CO.site_tile(S) == tile
        ctx.set_leaves(g)
        ctx.set_model(Q, PI, lam, lam)
        ref = CO.sweep(g, Q, PI, lam, lam, K, 3, want_nodes=True)
        what = "S=%d T=%d %s" % (S, tile, kinds)
        counts = classes_of(ref, PI, tile, need, what)
        lw = ref['log_weights']
        if kinds == SC.FINITE:
            assert np.isfinite(lw).all() and math.isfinite(ref['logZ'])
        elif kinds == SC.ALLBAD:                               # every weight of every rank event is non-finite
            assert not np.isfinite(lw).any()
        elif kinds == SC.TILES:
            # no NaN factor anywhere: zeros and infinities decide results, and some row is NaN only because pk_tile_epilogue adds a
            # -inf tile value and a later +inf tile value
            x = SC.site_likelihoods(ref['nodes'], PI)
            assert not (np.isnan(x) | (x < 0)).any()
            assert len(SC.rows_decided_by_the_tile_sum(x, tile)) > 0
            ll = ref['log_likelihood']
            assert (ll == -math.inf).any() and (ll == math.inf).any() and np.isnan(ll).any() and np.isfinite(ll).any()
        elif S == 449:
            # the one-launch sweep's flag: in ONE rank event (the last) every particle of every workgroup holds specials, on many
            # lanes besides lane 7; earlier, particle by particle: some weights of a rank event finite, some not
            particles, lanes = SC.special_spread(SC.site_likelihoods(ref['nodes'][N - 2], PI))
            assert particles == K and len(set(lanes) - {7}) >= 2, (particles, lanes)
            if T == 0:
                flagged = [SC.special_spread(SC.site_likelihoods(ref['nodes'][r], PI))[0] for r in range(N - 1)]
                assert any(1 < f < K for f in flagged), flagged   # and a rank event where only some particles are redone
                assert any(np.isfinite(row).any() and not np.isfinite(row).all() for row in lw)
        for flags, name in FORMS:
            out = ctx.sweep(3, flags=flags)
            if flags & _ffi.ONE_LAUNCH:
                assert out['stats']['n_launches'] == 1, "the one-launch form did not run"
            check(out, ref, what + ", " + name)
            sample_nodes(ctx, ref, N, K, what + ", " + name)
        if kinds == SC.FINITE:                                 # the oracle's sum over its own node rows against 60 digits
            for (r, k) in [(N - 2, 0), (N - 2, K - 1), (2, 5)]:
                node = ref['nodes'][r, k][None, None]
                got = ctx.forest_loglik(node, np.ones((1, 1), dtype=np.int32))[0]
                assert same(got, CO.forest_loglik(PI, node, np.ones((1, 1), dtype=np.int32))[0])
                exact, bound = R.row_bound(SC.site_likelihoods_fma(ref['nodes'][r, k], PI), tile)
                assert abs(mp.mpf(float(got)) - exact) <= bound, (r, k, got, float(abs(mp.mpf(float(got)) - exact)), bound)
    finally:
        CO.set_site_tile(0)
        if ctx is not None:
            ctx.close()


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("leaves", ["generic", "coded"])
def test_twisted_sweep_on_edge_rows(leaves, M):
    """pk_twist_adopt_draws, pk_twist_potentials (pk_rows_v4 for a coded leaf against an internal root, pk_twist_potentials_ll's
    code-pair pricing for two coded leaves), then the ordinary merge: bit for bit the oracle's twisted sweep.  The replay covers the
    merged nodes; the look-ahead potentials price every pair of roots of every particle, a superset of them.  Under expm at rates
    of 1e155 a leaf x leaf f_c is about 1e-156, a positive normal number: these cases give pk_twist_potentials_ll small but ordinary
    code pairs only (its special values are the next test's)."""
    N, K = 6, 48
    if leaves == "generic":
        S = 449
        g = SC.scaled_leaves(N, S, 2048, SC.SPECIAL, seed=4)
        lam = np.full(N - 1, 10.0)
        need = PAIR_CLASSES + ('first', 'second', 'last', 'col0', 'col63')
    else:
        S = 200
        g = SC.coded_leaves(N, S, seed=2)
        lam = np.full(N - 1, 1e155)
        need = SC.CODED_NEED
    Q = generic_Q()
    ref = CO.sweep_twisted(g, Q, PI, lam, lam, K, M, 7, want_nodes=True)
    classes_of(ref, PI, 2048, need, "twisted %s M=%d" % (leaves, M))
    assert not np.isfinite(ref['log_weights']).all()
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, PI, lam, lam)
        out = ctx.sweep(7, flags=_ffi.FLAGS_DEFAULT | _ffi.TWISTING, M=M)
        check(out, ref, "twisted %s M=%d" % (leaves, M))
        sample_nodes(ctx, ref, N, K, "twisted %s M=%d" % (leaves, M))


def test_twisted_coded_jc69_prices_zero_code_pairs():
    """pk_twist_potentials_ll's code-pair pricing, sum_c count_c log f_c, with a special f_c: under the JC69 closed form at rates of
    1e155 the off-diagonal transition probabilities are exactly 0, so f_c = 0 for every mismatching pair of codes and the potential
    of every pair of leaves is -inf -- asserted from the oracle's potentials at rank event 0, where every root is a leaf.  The
    choice among potentials that are all -inf, the merges and the resampling indices must be the oracle's."""
    N, S, K = 6, 200, 48
    g = SC.coded_leaves(N, S, seed=2)
    lam = np.full(N - 1, 1e155)
    Q = O.jc_Q()
    for M in (1, 3):
        ref = CO.sweep_twisted(g, Q, PI, lam, lam, K, M, 7, jc=True, want_nodes=True, want_potentials=True)
        assert (CO.expm_batched(Q, ref['left_branches'][0], jc=True) == np.eye(4)).all()
        assert np.isneginf(ref['potentials'][0][:, :M * N * (N - 1) // 2]).all()
        classes_of(ref, PI, 2048, ('kept', 'x1', 'x2', 'first', 'second', 'last', 'col0', 'col63'), "twisted coded JC69 M=%d" % M)
        with _ffi.Context(K, N, S) as ctx:
            ctx.set_leaves(g)
            ctx.set_model(Q, PI, lam, lam, jc69_closed_form=True)
            out = ctx.sweep(7, flags=_ffi.FLAGS_DEFAULT | _ffi.TWISTING, M=M)
            check(out, ref, "twisted coded JC69 M=%d" % M)
            sample_nodes(ctx, ref, N, K, "twisted coded JC69 M=%d" % M)


@pytest.mark.parametrize("jc", [False, True], ids=["expm", "jc69"])
def test_sweep_forms_on_coded_leaves_with_extreme_rates(jc):
    """pk_rows_run<true,*> and the 25-entry leaf x leaf table: every form against the oracle."""
    N, S, K = 6, 200, 64
    g = SC.coded_leaves(N, S, seed=2)
    lam = np.full(N - 1, 1e155)
    Q = O.jc_Q() if jc else generic_Q()
    ref = CO.sweep(g, Q, PI, lam, lam, K, 3, jc=jc, want_nodes=True)
    what = "coded leaves, rates 1e155, %s" % ("JC69 closed form" if jc else "expm")
    classes_of(ref, PI, 2048, ('kept', 'x1', 'x2', 'first', 'second', 'last', 'col0', 'col63') if jc else SC.CODED_NEED, what)
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, PI, lam, lam, jc69_closed_form=jc)
        for flags, name in FORMS:
            out = ctx.sweep(3, flags=flags)
            check(out, ref, what + ", " + name)
            sample_nodes(ctx, ref, N, K, what + ", " + name)


def test_batched_groups_on_edge_rows():
    """three groups in one set of launches, in both forms: each group is bit for bit the sweep of its seed run alone, although
    specials strike different particles at different rank events in each."""
    N, S, Kg = 6, 449, 32
    g = SC.scaled_leaves(N, S, 2048, SC.SPECIAL, seed=1)
    Q = generic_Q()
    lam = np.full(N - 1, 10.0)
    seeds = [3, 50, 51]
    refs = [CO.sweep(g, Q, PI, lam, lam, Kg, s, want_nodes=True) for s in seeds]
    for s, ref in zip(seeds, refs):
        classes_of(ref, PI, 2048, PAIR_CLASSES + ('last',), "group of seed %d" % s)
    patterns = {np.isfinite(r['log_weights']).tobytes() for r in refs}
    assert len(patterns) == 3                                  # the groups do not go bad alike
    with _ffi.Context(3 * Kg, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, PI, lam, lam)
        for fl in (_ffi.ONE_LAUNCH, 0):
            ctx.sweep_batch_async(seeds, flags=_ffi.FLAGS_DEFAULT | fl)
            out = ctx.sweep_fetch()
            logz = ctx.sweep_fetch_logz(3)
            for key in ('log_weights', 'log_likelihood', 'left_branches', 'right_branches'):
                assert same(out[key], np.concatenate([r[key] for r in refs], axis=1)), (fl, key)
            np.testing.assert_array_equal(out['ancestors'], np.concatenate([r['ancestors'] for r in refs], axis=1))
            np.testing.assert_array_equal(out['merges'], np.concatenate([r['merges'] for r in refs], axis=1))
            assert same(logz, [r['logZ'] for r in refs])
    with _ffi.Context(Kg, N, S) as ctx:                        # ... and of this library's
        ctx.set_leaves(g)
        ctx.set_model(Q, PI, lam, lam)
        for s, ref in zip(seeds, refs):
            check(ctx.sweep(s), ref, "seed %d alone" % s)
