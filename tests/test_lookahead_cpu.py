"""The twisted proposal's look-ahead lists of the reverse pass (phylo_amd/csrc/phylo_revlists.h: pg_build_lookahead) against a plain
restatement in Python, on random adopted root tables from flat to degenerate and in both chunk regimes.  No GPU:
phylo_debug_lookahead_lists runs the function phylo_sweep_backward calls."""
import numpy as np
import pytest

from phylo_amd import _ffi

XCH = 16                              # PG_XCH (phylo_grad.h): most entries of a chunk
START = 1 << 30                       # xnode_nchunks: this record's pg_twist_xsum starts the node's adjoint row


def _random_roots(rng, N, K, survivors, p_internal):
    """adopted root tables [N-1][K][N]: slot i < N - r of rank event r holds a leaf or a node of an earlier rank event, drawn from
    about `survivors` distinct nodes (few: a degenerate genealogy; K (N-1): flat); the slots beyond are never read"""
    R = N - 1
    rad = np.full((R, K, N), 1 << 29, dtype=np.int32)
    for r in range(R):
        n = N - r
        rad[r, :, :n] = rng.integers(0, N, size=(K, n))
        if r == 0:
            continue
        pool = N + rng.choice(r * K, size=min(survivors, r * K), replace=False)
        w = rng.dirichlet(np.full(len(pool), 0.3))
        pick = rng.choice(pool, size=(K, n), p=w)
        internal = rng.random((K, n)) < p_internal
        rad[r, :, :n] = np.where(internal, pick, rad[r, :, :n])
    return rad


def _reference(N, K, S, rad):
    """per rank event: {node: entries ascending}, and the chunk shape (entries per chunk, partner slots per slice)"""
    R = N - 1
    target = max(64, 2048 // ((S + 255) // 256))
    events = []
    for r in range(R):
        n = N - r
        ent = {}
        if r > 0:
            for k in range(K):
                for i in range(n):
                    x = int(rad[r, k, i])
                    if x >= N:
                        ent.setdefault(x, []).append(k * N + i)
        total = sum(len(v) for v in ent.values())
        xch = min(max(-(-total // target), 1), XCH)
        slices = 1
        if xch == 1 and total > 0:
            slices = min(max(target // total, 1), n)
        pw = -(-n // slices)
        events.append((ent, xch, pw))
    return events


CASES = [
    # N, K, S, M, survivors, p_internal, seed
    (2, 4, 64, 1, 1, 0.5, 0), (2, 4, 64, 10, 1, 0.5, 0), (3, 5, 64, 1, 2, 0.7, 1), (3, 5, 64, 10, 100, 0.7, 2),
    (8, 32, 256, 10, 3, 0.5, 3),          # few entries: one per chunk, partner slots one per slice
    (8, 64, 256, 1, 1000, 0.5, 4),        # ... flat
    (10, 128, 256, 10, 5, 0.5, 5),        # one entry per chunk, several partner slots per slice
    (10, 300, 256, 1, 8, 0.6, 6),         # one entry per chunk, one slice
    (8, 512, 898, 1, 4, 0.6, 7),          # several entries per chunk
    (6, 2048, 2000, 10, 3, 0.7, 8),       # PG_XCH entries per chunk, degenerate
    (6, 2048, 2000, 1, 100000, 0.7, 9),   # ... flat
    (7, 40, 5000, 1, 2, 0.05, 10),        # hardly any internal root; the floor of 64 workgroups
    (5, 16, 128, 1, 3, 0.0, 11),          # leaves only
]


def _check_case(N, K, S, M, survivors, p_internal, seed):
    """checks one case against the restatement; returns the chunk shapes it met: entries per chunk, slices per entry run"""
    rng = np.random.default_rng(seed)
    R = N - 1
    rad = _random_roots(rng, N, K, survivors, p_internal)
    flag0 = (rng.integers(0, 2, size=R * K) * 4 + rng.integers(0, 2, size=R * K)).astype(np.int32)   # bits 0 and 2 are others'
    out = _ffi.debug_lookahead_lists(N, K, S, M, rad, flag0)
    events = _reference(N, K, S, rad)
    seen_xch, seen_slices = set(), set()
    touched = {}                          # node -> newest rank event that touches it
    n_ent = n_chunks = n_nodes = max_chunks = 0
    for r, (ent, xch, pw) in enumerate(events):
        n = N - r
        assert out["ev_chunk0"][r] == n_chunks and out["ev_node0"][r] == n_nodes
        ids = out["xnode_id"][n_nodes:n_nodes + len(ent)]
        assert list(ids) == sorted(ent), r           # the touched nodes of the rank event, ascending
        for j, x in enumerate(sorted(ent)):
            rec = n_nodes + j
            c0, nc = int(out["xnode_chunk0"][rec]), int(out["xnode_nchunks"][rec]) & ~START
            assert c0 == n_chunks
            want = ent[x]
            assert want == sorted(want)              # adopters ascending (entry = adopter * N + slot)
            # every (adopter, slot) entry once under its node
            assert list(out["xent"][n_ent:n_ent + len(want)]) == want, (r, x)
            # the chunks partition entries x partner slots: runs of up to xch entries, each with slices of pw partner slots
            cover = np.zeros((len(want), n), dtype=np.int32)
            expect = [(n_ent + b, min(xch, len(want) - b), p0, min(p0 + pw, n)) for b in range(0, len(want), xch) for p0 in range(0, n, pw)]
            assert nc == len(expect)
            for q, (beg, cnt, p0, p1) in enumerate(expect):
                ch = c0 + q
                assert out["xchunk_node"][ch] == x
                part = int(out["xchunk_part"][ch])
                assert (int(out["xchunk_beg"][ch]), int(out["xchunk_cnt"][ch]), part & 0xffff, part >> 16) == (beg, cnt, p0, p1), (r, x, q)
                assert 1 <= cnt <= XCH and 0 <= p0 < p1 <= n
                cover[beg - n_ent:beg - n_ent + cnt, p0:p1] += 1
            assert (cover == 1).all(), (r, x)
            n_ent += len(want)
            n_chunks += nc
            touched[x] = r
        if ent:
            seen_xch.add(xch)
            seen_slices.add(-(-n // pw))
        n_nodes += len(ent)
        max_chunks = max(max_chunks, n_chunks - int(out["ev_chunk0"][r]))
    assert out["ev_chunk0"][R] == n_chunks == out["n_xchunks"] and out["ev_node0"][R] == n_nodes == out["n_xnodes"]
    assert out["n_xent"] == n_ent and out["tw_max_chunks"] == max_chunks
    # bit 30 on exactly one record per node: that of the newest rank event that touches it
    for r in range(R):
        for rec in range(int(out["ev_node0"][r]), int(out["ev_node0"][r + 1])):
            x = int(out["xnode_id"][rec])
            assert bool(int(out["xnode_nchunks"][rec]) & START) == (touched[x] == r), (r, x)
            assert (int(out["xnode_nchunks"][rec]) & ~START) >= 1          # a record that owns chunks
    # bit 1 of slow_flag for exactly the touched nodes; the other bits stay
    want_flag = flag0.copy()
    for x in touched:
        want_flag[x - N] |= 2
    assert np.array_equal(out["slow_flag"], want_flag)
    return seen_xch, seen_slices


@pytest.mark.parametrize("N,K,S,M,survivors,p_internal,seed", CASES)
def test_lookahead_lists_match_restatement(N, K, S, M, survivors, p_internal, seed):
    _check_case(N, K, S, M, survivors, p_internal, seed)


def test_both_chunk_regimes_are_reached():
    by_seed = {c[-1]: c for c in CASES}
    xch, _ = _check_case(*by_seed[8])
    assert XCH in xch                                     # many entries: up to PG_XCH per chunk, all partner slots
    xch, slices = _check_case(*by_seed[3])
    assert xch == {1} and max(slices) > 1                 # few entries: one per chunk, the partner slots in slices
    xch, slices = _check_case(*by_seed[7])
    assert 1 < max(xch) < XCH and slices == {1}


def test_lists_do_not_depend_on_M():
    rad = _random_roots(np.random.default_rng(12), 7, 48, 4, 0.5)
    a, b = _ffi.debug_lookahead_lists(7, 48, 300, 1, rad), _ffi.debug_lookahead_lists(7, 48, 300, 10, rad)
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def test_bad_arguments_are_refused():
    rad = np.zeros((2, 4, 3), np.int32)
    with pytest.raises(_ffi.PhyloError):
        _ffi.debug_lookahead_lists(3, 4, 64, 0, rad)                   # M < 1
    with pytest.raises(_ffi.PhyloError):
        _ffi.debug_lookahead_lists(3, 4, 0, 1, rad)                    # S < 1
    bad = rad.copy()
    bad[1, 0, 0] = 3 + 4                                               # a node of rank event 1 among rank event 1's roots
    with pytest.raises(_ffi.PhyloError):
        _ffi.debug_lookahead_lists(3, 4, 64, 1, bad)
    bad[1, 0, 0] = -1
    with pytest.raises(_ffi.PhyloError):
        _ffi.debug_lookahead_lists(3, 4, 64, 1, bad)
