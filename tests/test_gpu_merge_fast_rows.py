"""pk_rank_merge_nostore's row loops for tiles that start on a chunk boundary -- a chunk's steps walked at constant shifts, the running
product updated speculatively (pm_lp_mul2_spec), a flagged wave recomputed by the general path -- bit for bit against the C oracle's
sweep: ancestors, merges, the four float arrays as uint64, log Z-hat.  The shapes are the smallest at which the loops can go wrong:
every count of steps at which a chunk's walk ends differently, tiles of several chunks, a tile that starts mid-chunk (the general
path from the start), launches in which flagged and clean waves run side by side, and leaf x leaf tables with entries that are not
positive normal numbers.  No tolerances."""
import functools

import numpy as np
import pytest

import packed_codes_cases as PC
from tests import site_product_cases as SC
from tests import site_product_ref as R
from oracle import c_oracle as CO
from oracle import cpu_ref as O
from phylo_amd import _ffi

gpu = pytest.mark.gpu
FLOATS = ('log_weights', 'log_likelihood', 'left_branches', 'right_branches')
PI = np.array([[0.1, 0.2, 0.3, 0.4]])
N0, K0 = 5, 64


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def gtr():
    return O.get_Q(O.init_y_q())


def lam(N, v=10.0):
    return np.full(N - 1, v)


def same(out, logz, ref, what, sl=slice(None)):
    np.testing.assert_array_equal(out['ancestors'][:, sl], ref['ancestors'], err_msg=what)
    np.testing.assert_array_equal(out['merges'][:, sl], ref['merges'], err_msg=what)
    for key in FLOATS:
        got = out[key][:, sl]
        eq = (bits(got) == bits(ref[key])) | (np.isnan(got) & np.isnan(ref[key]))
        bad = np.argwhere(~eq)
        assert len(bad) == 0, "%s: %s: %d of %d differ, first at %s: %r against %r" % (
            what, key, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], ref[key][tuple(bad[0])])
    lz, rz = np.float64(logz), np.float64(ref['logZ'])
    assert bits(lz) == bits(rz) or (np.isnan(lz) and np.isnan(rz)), "%s: log Z %r against %r" % (what, logz, ref['logZ'])


def uses_record(N, K, S, G=1):
    return _ffi.debug_sweep_plan(N, K, S, G=G, flags=_ffi.FLAGS_DEFAULT)['use_rec']


def check(g, K, seed, what, tile=0):
    """One sweep of alignment g on a fresh context against the oracle's, both at site tile `tile` (0: the default)."""
    N, S, _ = g.shape
    assert uses_record(N, K, S), what
    Q = gtr()
    ctx = _ffi.Context(K, N, S)
    try:
        ctx.set_leaves(g)
        ctx.set_model(Q, PI, lam(N), lam(N))
        if tile:
            ctx.set_site_tile(tile)
            CO.set_site_tile(tile)
        ref = CO.sweep(g, Q, PI, lam(N), lam(N), K, seed)
        out = ctx.sweep(seed)
        same(out, out['logZ'], ref, what)
    finally:
        if tile:
            CO.set_site_tile(0)
        ctx.close()


@gpu
@pytest.mark.parametrize("S", [64, 128, 129, 192, 961, 1023, 1024])
def test_step_counts_inside_one_chunk(S):
    """1 step; one pair; a pair plus a lone lane (an odd last step); 3 steps; 16 steps with the last one partial, at one lane (961)
    and at 63 (1023); a full chunk."""
    check(PC.genome(PC.edge_codes(N0, S, seed=S + 7)), K0, 5, "S=%d" % S)


@gpu
@pytest.mark.parametrize("S,T", [(1025, 0), (1088, 0), (2049, 0), (2100, 1024)])
def test_chunk_aligned_tiles_of_several_chunks(S, T):
    """A second chunk of one step, with one lane and with all of them; the default tile with a second tile of one site; three
    aligned tiles of one chunk each (the last of 52 sites)."""
    if T == 0:
        assert _ffi.load().phylo_site_tile(S) == 2048
    else:
        assert T % 1024 == 0                               # every tile starts on a chunk boundary
    check(PC.genome(PC.edge_codes(N0, S, seed=S + 3)), K0, 6, "S=%d T=%d" % (S, T), tile=T)


@gpu
def test_mid_chunk_tile_takes_the_general_path():
    """T = 192: tiles 1 to 5 start inside the first chunk (tile 5, steps 15 to 17, crosses into the second); tile 0 is aligned."""
    S, T = 1100, 192
    assert any((t * T) % 1024 for t in range(-(-S // T)))
    check(PC.genome(PC.edge_codes(N0, S, seed=41)), K0, 6, "S=%d T=%d" % (S, T), tile=T)


# ---- the redo: flagged and clean waves in ONE launch ------------------------------------------------------------------------------
# Coded leaves under GTR at rates of 1e155: a leaf x leaf site whose codes differ has a likelihood of about 1e-156 -- a normal number,
# but two of them in one pair of steps of one column underflow the pair's product q, which pm_lp_mul2 rejects ('small').  All
# leaves share one random sequence; leaves 2 .. N - 1 differ from it, and from each other (but 2 and 5), at sites C and C + 64: steps
# 0 and 1 of column C, one pair.  Leaves 0 and 1 are identical at every site, so their merge is clean; so is (0, 2)'s neighbour
# (2, 5).  Every other pair of leaves, and every merge that joins differing codes at those sites later, flags.
RN, RS, RK, RC = 6, 200, 64, 5


@functools.lru_cache(maxsize=None)
def redo_case():
    base = np.random.default_rng(9).integers(0, 4, RS).astype(np.uint8)
    codes = np.tile(base, (RN, 1))
    for i in range(2, RN):
        for s in (RC, RC + 64):
            codes[i, s] = (base[s] + 1 + (i - 2) % 3) % 4
    assert (codes[0] == codes[1]).all()
    g = PC.genome(codes)
    refs = {sd: CO.sweep(g, gtr(), PI, lam(RN, 1e155), lam(RN, 1e155), RK, sd, want_nodes=True) for sd in (3, 11)}
    return g, refs


def fallback_rows(x, T=2048):
    """x [K, S]: site likelihoods of the K new nodes of one rank event -> for every particle, whether some pair of steps of some
    column takes pm_lp_mul2's fall-back, or an odd last step holds a factor that is not a positive normal number."""
    K, S = x.shape
    hit = np.zeros(K, dtype=bool)
    for s0 in range(0, S, T):
        s1 = min(s0 + T, S)
        steps = (s1 - s0 + 63) // 64
        tile = np.ones((K, steps * 64))
        tile[:, :s1 - s0] = x[:, s0:s1]
        tile = tile.reshape(K, steps, 64)
        p = np.ones((K, 64))
        for j in range(0, steps - 1, 2):
            hit |= (R.branch_of(p, tile[:, j], tile[:, j + 1]) != 0).any(axis=1)
            p = R.lp_two_np(p, tile[:, j], tile[:, j + 1], lambda v: np.zeros(v.shape))[0]
        if steps % 2 == 1:
            last = tile[:, steps - 1]
            hit |= (~((last >= R.TINY) & (last <= R.MAXF))).any(axis=1)
    return hit


def mixed_rank_events(ref, N):
    """rank events at which particles WITH a fall-back and particles WITHOUT one both occur"""
    out = []
    for r in range(N - 1):
        hit = fallback_rows(SC.site_likelihoods(ref['nodes'][r], PI))
        if hit.any() and not hit.all():
            out.append((r, int(hit.sum())))
    return out


def test_redo_inputs_reach_both_paths_at_one_rank_event():
    """No GPU: the oracle alone.  In both seeds some rank event has flagged and clean merges side by side -- at rank event 0 (all
    leaf x leaf) and at a later one (merges with an internal child)."""
    _, refs = redo_case()
    assert R.BRANCHES[0] == 'kept'
    for sd, ref in refs.items():
        ev = mixed_rank_events(ref, RN)
        print("seed", sd, ev)
        assert ev and ev[0][0] == 0, ev
        assert any(r > 0 for r, _ in ev), ev
        assert np.isfinite(ref['logZ'])


@gpu
def test_redo_with_flagged_and_clean_waves_in_one_launch():
    g, refs = redo_case()
    assert uses_record(RN, RK, RS)
    assert mixed_rank_events(refs[3], RN)
    with _ffi.Context(RK, RN, RS) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(gtr(), PI, lam(RN, 1e155), lam(RN, 1e155))
        out = ctx.sweep(3)
        same(out, out['logZ'], refs[3], "redo, one sweep")


@gpu
def test_redo_in_batched_groups():
    """The same inputs as G = 2 groups in one launch set: each group against the oracle's sweep of its own seed."""
    g, refs = redo_case()
    seeds = [3, 11]
    assert uses_record(RN, 2 * RK, RS, G=2)
    with _ffi.Context(2 * RK, RN, RS) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(gtr(), PI, lam(RN, 1e155), lam(RN, 1e155))
        ctx.sweep_batch_async(seeds)
        out = ctx.sweep_fetch()
        logz = ctx.sweep_fetch_logz(2)
    for i, sd in enumerate(seeds):
        same(out, logz[i], refs[sd], "redo, group %d" % i, slice(i * RK, (i + 1) * RK))


@gpu
def test_special_table_entries_under_the_jc69_closed_form():
    """JC69's closed form at rates of 1e155: 1/4 - 1/4 exp(-t) is exactly 0, so the lik25 entries of differing codes are zeros.  A
    leaf x leaf wave must take the general loop up front (its fast loop does not test its factors); a mixed merge meets the zeros
    as factors, flags and is redone."""
    N, S, K = 6, 200, 64
    g = SC.coded_leaves(N, S, seed=2)
    pi = np.full((1, 4), 0.25)
    Q = O.jc_Q()
    ref = CO.sweep(g, Q, pi, lam(N, 1e155), lam(N, 1e155), K, 3, jc=True, want_nodes=True)
    x0 = SC.site_likelihoods(ref['nodes'][0], pi)
    assert (x0 == 0).any(axis=1).all()                     # every leaf x leaf merge of rank event 0 reads a zero entry
    assert any(fallback_rows(SC.site_likelihoods(ref['nodes'][r], pi)).any() for r in range(1, N - 1))
    assert uses_record(N, K, S)
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, pi, lam(N, 1e155), lam(N, 1e155), jc69_closed_form=True)
        out = ctx.sweep(3)
        same(out, out['logZ'], ref, "JC69 closed form, rates 1e155")
