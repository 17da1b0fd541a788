"""Oracle of the branch lengths of the tree posterior (phylo_tree_branches), NumPy and Python ints.

Builds on tests/tree_posterior_ref.py: every particle's tree comes from the sweep's FETCHED merges and ancestors replayed through
the root tables (the device's children records and its walk are never read), and the length of the branch above every node from
the fetched left_branches / right_branches carried through the same replay.  The canonical segment sum (element j to column
j mod 64, columns added in increasing j from +0.0, the 64 columns by the adjacent-pair tree) is restated here in NumPy."""
import math
from fractions import Fraction

import numpy as np

import tree_posterior_ref as REF
from phylo_amd import rng


def particle_branches(N, K, merges, ancestors, lb, rb, seed, twisted):
    """[K] dicts of every final particle's tree: key = clade bitset (Python int, leaf i = 1 << i, the root absent) ->
    (rank event that made the node, or -1 for a leaf; length of the branch above it)"""
    R = N - 1
    tab = [[(1 << i, {}) for i in range(N)] for _ in range(K)]      # per root slot: (bitset, branches finished below it)
    made = [{} for _ in range(K)]                                   # per particle: bitset -> rank event (carried alike)
    for r in range(R):
        if r > 0:
            idx = [int(i) for i in ancestors[r - 1]]
            tab = [tab[i] for i in idx]
            made = [made[i] for i in idx]
        if twisted:
            rems = [[i for i in range(N - r - 1, -1, -1) if i != a and i != b] for a, b in merges[r]]
        else:
            co, rems = rng.pair_order(K, N - r, seed, r)
            assert np.array_equal(co, merges[r]), "host replay of the pair pick disagrees with the device"
        ntab, nmade = [], []
        for k in range(K):
            a, b = int(merges[r][k][0]), int(merges[r][k][1])
            (ba, da), (bb, db) = tab[k][a], tab[k][b]
            d = dict(da)
            d.update(db)
            d[ba] = float(lb[r][k])
            d[bb] = float(rb[r][k])
            m = dict(made[k])
            m[ba | bb] = r
            ntab.append([tab[k][int(i)] for i in rems[k]] + [(ba | bb, d)])
            nmade.append(m)
        tab, made = ntab, nmade
    out = []
    for k in range(K):
        (_, d), = tab[k]
        assert len(d) == 2 * N - 2
        out.append({c: (made[k].get(c, -1), b) for c, b in d.items()})
    return out


def canon_sum(vals):
    """the canonical segment sum of a 1-D float64 array (non-negative terms)"""
    v = np.asarray(vals, dtype=np.float64)
    rows = np.concatenate([v, np.zeros((-v.size) % 64)]).reshape(-1, 64)
    col = np.zeros(64)
    for row in rows:
        col = col + row
    while col.size > 1:
        col = col[0::2] + col[1::2]
    return col[0]


def stats(us, bs):
    """(S1, S2, min, max) of one segment: integer weights us, lengths bs, in the segment's order"""
    b = np.asarray(bs, dtype=np.float64)
    x = np.array([float(u) for u in us], dtype=np.float64) * b
    return canon_sum(x), canon_sum(x * b), b.min(), b.max()


def branch_tables(N, trees, u, summary):
    """phylo_tree_branches' tables of one group: trees from particle_branches, u and summary from tree_posterior_ref"""
    K = len(trees)
    W = summary['clade_bits'].shape[1]
    corder = [sum(int(row[w]) << (64 * w) for w in range(W)) for row in summary['clade_bits']]
    crow = {c: j for j, c in enumerate(corder)}
    holders = {}                                       # clade -> [(entry r K + k, k)] over the particles whose tree holds it
    for k, tree in enumerate(trees):
        for c, (r, _) in tree.items():
            if c & (c - 1):
                holders.setdefault(c, []).append((r * K + k, k))
    clade_stats = np.empty((len(corder), 4))
    members = []
    for j, c in enumerate(corder):
        ks = [k for _, k in sorted(holders[c])]        # ascending entry index
        clade_stats[j] = stats([u[k] for k in ks], [trees[k][c][1] for k in ks])
        members.append(ks)
    leaf_stats = np.array([stats(u, [trees[k][1 << i][1] for k in range(K)]) for i in range(N)])
    nt = len(summary['topo_weight'])
    of_topo = [[] for _ in range(nt)]
    for k, t in enumerate(np.asarray(summary['particle_topo'])):
        of_topo[int(t)].append(k)                      # ascending k
    topo_clades = np.empty((nt, N - 2), dtype=np.int32)
    topo_stats = np.empty((nt, 2 * N - 2, 4))
    for t, ks in enumerate(of_topo):
        rows = sorted(crow[c] for c in trees[ks[0]] if c & (c - 1))
        topo_clades[t] = rows
        keys = [1 << i for i in range(N)] + [corder[j] for j in rows]
        for q, c in enumerate(keys):
            topo_stats[t, q] = stats([u[k] for k in ks], [trees[k][c][1] for k in ks])
    return {'clade_stats': clade_stats, 'leaf_stats': leaf_stats, 'topo_clades': topo_clades, 'topo_stats': topo_stats,
            'clade_members': members, 'topo_members': of_topo, 'clade_keys': corder}


def expected(out, N, K, seed, twisted=False):
    """(summary tables, branch tables, trees, u) of one fetched sweep"""
    clades = REF.particle_clades(N, K, out['merges'], out['ancestors'], seed, twisted)
    u = REF.int_weights(out['log_weights'][N - 2])
    summary = REF.summarise(N, clades, u)
    trees = particle_branches(N, K, out['merges'], out['ancestors'], out['left_branches'], out['right_branches'], seed, twisted)
    for k in range(K):
        assert {c for c in trees[k] if c & (c - 1)} == set(clades[k]), "the two replays disagree on particle %d" % k
    return summary, branch_tables(N, trees, u, summary), trees, u


def assert_branches_equal(got, exp, what=""):
    for key in ('clade_stats', 'leaf_stats', 'topo_stats'):
        g, e = np.ascontiguousarray(got[key], dtype=np.float64), np.ascontiguousarray(exp[key], dtype=np.float64)
        assert g.shape == e.shape, "%s %s: %r against %r" % (what, key, g.shape, e.shape)
        assert not np.isnan(g).any(), "%s %s holds NaN" % (what, key)
        np.testing.assert_array_equal(g.view(np.uint64), e.view(np.uint64), err_msg="%s %s" % (what, key))
    np.testing.assert_array_equal(np.asarray(got['topo_clades']), np.asarray(exp['topo_clades']), err_msg="%s topo_clades" % what)


def exact_sums(us, bs):
    """(sum u b, sum u b b) exactly, as Fractions of the exact products"""
    s1 = s2 = Fraction(0)
    for u_, b in zip(us, bs):
        f = Fraction(float(b))
        s1 += int(u_) * f
        s2 += int(u_) * f * f
    return s1, s2


def bound(n):
    """relative error bound of a canonical segment sum of n non-negative terms against the exact sum: a column is a recursive
    sum of ceil(n / 64) terms, the tree adds 6 levels, the products 2 roundings"""
    return (math.ceil(n / 64) + 8) * 2.0 ** -53
