"""The one branch pass that is wide by size (tests/test_gpu_tree_branches_wide.py::test_wide_by_size), and a reference fast enough
for it.  Shared with tests/test_tree_branches_wide_cpu.py, which pins both without a GPU.

The shape.  (topology row << cbits | clade row) needs more than 32 bits only with very many distinct topologies AND clades, that
is with a particle system that does not collapse.  All-zero leaves give no finite log-weight at any rank event: by the contract
(all_bad) every draw is then uniform and every u_k = 1, so lineages coalesce only by chance.  (All-ONES leaves
do not do that: their likelihoods are finite and differ with the branch lengths, and the oracle's sweep of np.ones((24, 8, 4)) at
K = 65536 ends on 54 topologies and 145 clades.)  With N = 24, K = 65536, S = 8 the oracle's sweep of seed 1 ends on 142596 clades
and 36558 topologies: cbits 18 + tbits 16 = 34.  Topology rows from 2^15 on set key bit 33, clade rows from 2^14 on reach bit 32
through the shift.

The reference.  tests/tree_branches_ref.py holds a Python dict per particle and sums every segment in a Python loop: 16.5 s for
the trees and about 100 us per segment at this shape (1.8 million segments).  fast_expected restates the same rules on NumPy
arrays -- the same replay of the FETCHED merges and ancestors through the root tables, the same entry order inside a clade segment
(ascending r K + k), the same canonical segment sum -- for one bitset word and the plain proposal, and the CPU test holds it to
tree_branches_ref bit for bit at small shapes that have segments of 1, 64, 65, 200 and 256 elements and particles of weight 0.
Measured at the shape above, without a GPU: the replay 2.2 s, REF.summarise 1.9 s, the tables with ALL 36558 topology rows 3.3 s,
7.4 s together (2.5 s on the host of the MI355X the test ran on), so the GPU test compares every row of topo_stats and needs no
subset of rows."""
import numpy as np

import tree_posterior_ref as REF
from phylo_amd import rng

N, K, S, SEED = 24, 65536, 8, 1


def genome():
    return np.zeros((N, S, 4))


def segment_sums(x, starts, lens):
    """the canonical segment sum (tree_branches_ref.canon_sum) of every segment x[starts[i] : starts[i] + lens[i]] at once"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    starts, lens = np.asarray(starts, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    longest = int(lens.max()) if len(lens) else 0
    # (no segment longer than w <= 64 elements: columns w .. 63 stay +0.0, and the tree's levels above w add +0.0 to a
    #  non-negative sum, which changes no bit: w columns give the same result)
    w = 64 if longest > 32 else max(1, 1 << (longest - 1).bit_length())
    col = np.zeros((len(starts), w))
    lane = np.arange(w)[None, :]
    for t in range(-(-longest // 64)):
        act = np.flatnonzero(lens > 64 * t)
        off = 64 * t + lane                                 # element j = 64 t + column
        ok = off < lens[act, None]
        idx = np.where(ok, starts[act, None] + off, 0)
        col[act] = col[act] + np.where(ok, x[idx], 0.0)     # (what a shorter column adds is +0.0, as canon_sum's padding)
    while col.shape[1] > 1:
        col = col[:, 0::2] + col[:, 1::2]
    return col[:, 0]


def segment_stats(u, b, starts, lens):
    """[n_seg, 4]: S1 = sum of u b, S2 = sum of (u b) b, min b, max b (tree_branches_ref.stats) of every segment"""
    x = u * b
    out = np.empty((len(starts), 4))
    out[:, 0] = segment_sums(x, starts, lens)
    out[:, 1] = segment_sums(x * b, starts, lens)
    out[:, 2] = np.minimum.reduceat(b, starts)
    out[:, 3] = np.maximum.reduceat(b, starts)
    return out


def replay(N, K, out, seed):
    """Every final particle's tree from the fetched merges, ancestors and branch lengths (plain proposal, N <= 62): made [R, K],
    the clade of the node that the particle's ancestor at rank event r made; key [R, 2, K] and length [R, 2, K] of its children"""
    R = N - 1
    assert N <= 62
    anc = np.asarray(out['ancestors'], dtype=np.int64)
    tab = np.tile(np.int64(1) << np.arange(N, dtype=np.int64), (K, 1))
    rows = np.arange(K)
    A, B = [], []
    for r in range(R):
        if r > 0:
            tab = tab[anc[r - 1]]
        co, rem = rng.pair_order(K, N - r, seed, r)
        assert np.array_equal(co, out['merges'][r]), "host replay of the pair pick disagrees with the device"
        a, b = tab[rows, co[:, 0]], tab[rows, co[:, 1]]
        A.append(a)
        B.append(b)
        tab = np.concatenate([tab[rows[:, None], rem.astype(np.int64)], (a | b)[:, None]], axis=1)
    made, key, length = np.empty((R, K), dtype=np.int64), np.empty((R, 2, K), dtype=np.int64), np.empty((R, 2, K))
    lin = rows
    for r in range(R - 1, -1, -1):                          # lin: the final particle's ancestor at rank event r
        key[r, 0], key[r, 1] = A[r][lin], B[r][lin]
        length[r, 0], length[r, 1] = out['left_branches'][r][lin], out['right_branches'][r][lin]
        made[r] = key[r, 0] | key[r, 1]
        if r > 0:
            lin = anc[r - 1][lin]
    return made, key, length


def counts(N, K, out, seed):
    """(distinct clades, distinct topologies) over the final particles"""
    made, _, _ = replay(N, K, out, seed)
    cl = np.sort(made[:N - 2].T, axis=1)
    return len(np.unique(cl)), len(np.unique(cl, axis=0))


def fast_expected(out, N, K, seed):
    """(summary tables, branch tables) of one fetched sweep, as tree_branches_ref.expected gives them (without the members lists)"""
    R, L = N - 1, N - 2
    made, key, length = replay(N, K, out, seed)
    clades = [[int(c) for c in row] for row in made[:L][::-1].T]        # (REF.particle_clades lists the last rank event first)
    u = REF.int_weights(out['log_weights'][N - 2])
    summary = REF.summarise(N, clades, u)
    uf = np.array([float(x) for x in u])
    corder = summary['clade_bits'][:, 0].astype(np.int64)
    by_clade = np.argsort(corder)
    # the children of every tree: N leaves and N - 2 clades, each exactly once
    ck, cl = key.transpose(2, 0, 1).reshape(K, 2 * R), length.transpose(2, 0, 1).reshape(K, 2 * R)
    is_leaf = (ck & (ck - 1)) == 0
    assert (is_leaf.sum(axis=1) == N).all()
    order = np.argsort(np.where(is_leaf, ck, np.iinfo(np.int64).max), axis=1, kind='stable')[:, :N]
    leaf_len = np.take_along_axis(cl, order, axis=1)                    # [K, N]: the branch above leaf i (keys 1 << i ascend with i)
    assert (np.take_along_axis(ck, order, axis=1) == (np.int64(1) << np.arange(N, dtype=np.int64))[None, :]).all()
    # the branch above the clade made at rank event r of tree k: the child record of that tree with the same key
    order = np.argsort(np.where(is_leaf, np.iinfo(np.int64).max, ck), axis=1, kind='stable')[:, :L]
    child_key, child_len = np.take_along_axis(ck, order, axis=1), np.take_along_axis(cl, order, axis=1)   # ascending key
    mk = made[:L].T                                                     # [K, L] by rank event
    by_key = np.argsort(mk, axis=1, kind='stable')
    assert (np.take_along_axis(mk, by_key, axis=1) == child_key).all(), "a tree's clades are not its non-leaf children"
    clade_len = np.empty((K, L))
    np.put_along_axis(clade_len, by_key, child_len, axis=1)             # [K, L]: above the clade made at rank event r
    crow = by_clade[np.searchsorted(corder[by_clade], mk)]              # [K, L] output row of that clade
    assert (corder[crow] == mk).all()
    # clade rows: segment j = the entries r K + k of clade j, ascending
    entry = (np.arange(L, dtype=np.int64)[None, :] * K + np.arange(K, dtype=np.int64)[:, None]).ravel()
    o = np.lexsort((entry, crow.ravel()))
    seg_row = crow.ravel()[o]
    starts = np.flatnonzero(np.r_[True, seg_row[1:] != seg_row[:-1]])
    lens = np.diff(np.r_[starts, seg_row.size])
    assert len(starts) == len(corder) and (seg_row[starts] == np.arange(len(corder))).all()
    clade_stats = segment_stats(uf[entry[o] % K], clade_len.ravel()[o], starts, lens)
    # leaf rows: every particle, ascending
    leaf_stats = segment_stats(np.tile(uf, N), np.ascontiguousarray(leaf_len.T).ravel(), np.arange(N) * K, np.full(N, K))
    # topology rows: the particles of row t ascending; its clades by ascending output row
    pt = np.asarray(summary['particle_topo'], dtype=np.int64)
    perm = np.argsort(pt, kind='stable')
    nt = len(summary['topo_weight'])
    tstarts = np.searchsorted(pt[perm], np.arange(nt))
    tlens = np.diff(np.r_[tstarts, K])
    by_row = np.argsort(crow, axis=1, kind='stable')
    rows_sorted = np.take_along_axis(crow, by_row, axis=1)
    topo_clades = rows_sorted[perm[tstarts]].astype(np.int32)
    assert (rows_sorted[perm] == np.repeat(topo_clades, tlens, axis=0)).all(), "particles of one topology row differ in their clades"
    cols = np.concatenate([leaf_len, np.take_along_axis(clade_len, by_row, axis=1)], axis=1)[perm]        # [K, 2N - 2]
    topo_stats = np.stack([segment_stats(uf[perm], np.ascontiguousarray(cols[:, q]), tstarts, tlens) for q in range(2 * N - 2)], axis=1)
    return summary, {'clade_stats': clade_stats, 'leaf_stats': leaf_stats, 'topo_clades': topo_clades, 'topo_stats': topo_stats}
