"""pk_rank_merge_nostore reading a coded leaf's sites as packed per-lane code words (phylo_amd/csrc/phylo_packed_codes.h: one
16-byte load per lane serves 16 steps of 64 sites), bit for bit against the C oracle's sweep -- ancestors, merges, the four float
arrays as uint64, log Z-hat -- at the edges of a chunk, of the site tiles and of the image's lifetime.  Every case is one rank,
plain proposal, lazy nodes: the form that starts the merge from the particle's record (use_rec).  No tolerances."""
import numpy as np
import pytest

import packed_codes_cases as PC
from oracle import c_oracle as CO
from oracle import cpu_ref as O
from phylo_amd import _ffi
from phylo_amd.datasets import load_dataset

pytestmark = pytest.mark.gpu
FLOATS = ('log_weights', 'log_likelihood', 'left_branches', 'right_branches')
PI = np.array([[0.1, 0.2, 0.3, 0.4]])
N0, K0 = 5, 64


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def gtr():
    return O.get_Q(O.init_y_q())


def lam(N):
    return np.full(N - 1, 10.0)


def same(out, logz, ref, what, sl=slice(None)):
    np.testing.assert_array_equal(out['ancestors'][:, sl], ref['ancestors'], err_msg=what)
    np.testing.assert_array_equal(out['merges'][:, sl], ref['merges'], err_msg=what)
    for key in FLOATS:
        got = out[key][:, sl]
        bad = np.argwhere(bits(got) != bits(ref[key]))
        assert len(bad) == 0, "%s: %s: %d of %d differ, first at %s: %r against %r" % (
            what, key, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], ref[key][tuple(bad[0])])
    assert bits(logz) == bits(ref['logZ']), "%s: log Z %r against %r" % (what, logz, ref['logZ'])


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


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 127, 129, 1024, 1025, 1088])
def test_one_chunk_and_its_edges(S):
    """One lane, one step and its last lane, a second step of one lane, an odd and an even number of steps; exactly 16 steps
    (S = 1024: a whole chunk, no pad), a second chunk of one step with one lane (1025) and with all of them (1088)."""
    check(PC.genome(PC.edge_codes(N0, S, seed=S)), K0, 5, "S=%d" % S)


def test_primate_tail_step_with_two_lanes():
    """primate.p, 12 x 898: 15 steps, the last with two live lanes -- the flagship's row."""
    g = load_dataset('primate_data')['genome']
    assert g.shape[:2] == (12, 898)
    check(g, 128, 4, "primate.p")


@pytest.mark.parametrize("S,T", [(2049, 0), (200, 64), (1100, 192), (2300, 1088)])
def test_site_tiles(S, T):
    """The default tile with a second tile of one site; tiles of one step, each starting mid-chunk; a tile (5 of T = 192: steps 15
    to 17) that crosses a chunk boundary; a tile of 17 steps, the next starting at step 17."""
    if T == 0:
        assert _ffi.load().phylo_site_tile(S) == 2048
    check(PC.genome(PC.edge_codes(N0, S, seed=S + 1)), K0, 6, "S=%d T=%d" % (S, T), tile=T)


def test_batched_groups():
    """G = 2 groups of 64 in one launch set: every group against the oracle's sweep of its own seed."""
    N, S, G, Kg = N0, 129, 2, K0
    assert uses_record(N, G * Kg, S, G=G)
    g = PC.genome(PC.edge_codes(N, S, seed=77))
    Q = gtr()
    seeds = [31, 8]
    with _ffi.Context(G * Kg, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, PI, lam(N), lam(N))
        ctx.sweep_batch_async(seeds)
        out = ctx.sweep_fetch()
        logz = ctx.sweep_fetch_logz(G)
    for i, sd in enumerate(seeds):
        ref = CO.sweep(g, Q, PI, lam(N), lam(N), Kg, sd)
        same(out, logz[i], ref, "group %d" % i, slice(i * Kg, (i + 1) * Kg))


def test_uncoded_paths_stay_whole(monkeypatch):
    """The S = 129 case with the codes switched off, and with one row that is neither one-hot nor all-ones (the alignment has no
    codes): the record then carries row addresses and the merge reads rows."""
    S = 129
    g = PC.genome(PC.edge_codes(N0, S, seed=S))
    monkeypatch.setenv("PHYLO_NO_LEAF_CODES", "1")
    check(g, K0, 5, "codes switched off")
    monkeypatch.delenv("PHYLO_NO_LEAF_CODES")
    h = g.copy()
    h[3, 70] = [0.5, 0.5, 0.0, 0.0]
    check(h, K0, 5, "a row without a code")


def test_new_leaves_replace_the_packed_image():
    """Training on site minibatches: one context, leaves A, a sweep, leaves B that differ from A in every leaf, a sweep -- the
    second equals the oracle's for B."""
    N, S, K = N0, 129, K0
    assert uses_record(N, K, S)
    ca = PC.edge_codes(N, S, seed=1)
    cb = ca.copy()
    cb[:, ::3] = (cb[:, ::3] + 1) % 4                      # every leaf changes (leaf 1: from all gaps to a state)
    assert all((ca[i] != cb[i]).any() for i in range(N))
    A, B = PC.genome(ca), PC.genome(cb)
    Q = gtr()
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_model(Q, PI, lam(N), lam(N))
        for g, what in ((A, "leaves A"), (B, "leaves B")):
            ctx.set_leaves(g)
            out = ctx.sweep(12)
            same(out, out['logZ'], CO.sweep(g, Q, PI, lam(N), lam(N), K, 12), what)
