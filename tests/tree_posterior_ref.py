"""Oracle of the tree posterior summary (phylo_tree_summary), NumPy and Python ints.

Every particle's clades come from the sweep's FETCHED merges and ancestors, replayed through the root tables as
VCSMC._final_tables does (plain proposal: rng.pair_order; twisted: the remaining slots in descending order) -- the device's
children records are never read, so the device walk is checked independently.  Integer weights by the contract's exp
(oracle/c_oracle.math_probe op 0) and weights_prepare's rules; clade and topology weights as dict sums of Python ints."""
import numpy as np

from oracle import c_oracle as CO
from phylo_amd import rng


def int_weights(logw_last):
    """u_k = floor(exp(logw_k - max) 2^44); all-bad (no finite max): every u_k = 1; NaN: 0"""
    w = np.asarray(logw_last, dtype=np.float64)
    ok = ~np.isnan(w)
    m = w[ok].max() if ok.any() else -np.inf
    if not (m > -np.inf) or m == np.inf:
        return [1] * w.size
    with np.errstate(invalid='ignore'):
        e = CO.math_probe(0, np.where(ok, w - m, 0.0))
    return [int(np.float64(x) * np.float64(17592186044416.0)) if o else 0 for x, o in zip(e, ok)]


def particle_clades(N, K, merges, ancestors, seed, twisted):
    """[K] lists of the N-2 non-trivial clade bitsets (Python ints, taxon i = bit i) of every final particle's tree"""
    R = N - 1
    tab = np.empty((K, N), dtype=object)
    for i in range(N):
        tab[:, i] = 1 << i
    created = []                                       # created[r][k]: the clade of the node particle k made at rank event r
    rows = np.arange(K)[:, None]
    for r in range(R):
        if r > 0:
            tab = tab[np.asarray(ancestors[r - 1], dtype=np.int64)]
        if twisted:
            co = np.asarray(merges[r], dtype=np.int64)
            rem = np.array([[i for i in range(N - r - 1, -1, -1) if i != a and i != b] for a, b in co],
                           dtype=np.int64).reshape(K, N - r - 2)
        else:
            co, rem = rng.pair_order(K, N - r, seed, r)
            assert np.array_equal(co, merges[r]), "host replay of the pair pick disagrees with the device"
            co, rem = co.astype(np.int64), rem.astype(np.int64)
        new = tab[rows[:, 0], co[:, 0]] | tab[rows[:, 0], co[:, 1]]
        created.append(new)
        tab = np.concatenate([tab[rows, rem], new[:, None]], axis=1)
    clades = [[] for _ in range(K)]
    lin = np.arange(K)
    for r in range(R - 2, -1, -1):                     # the final particle's ancestor at rank event r
        lin = np.asarray(ancestors[r], dtype=np.int64)[lin]
        for k in range(K):
            clades[k].append(created[r][lin[k]])
    return clades


def summarise(N, clades, u):
    """the tables of phylo_tree_summary for one group, from per-particle clade lists and integer weights"""
    W = (N + 63) // 64
    U = sum(u)
    C, T, n, rep = {}, {}, {}, {}
    for k, cl in enumerate(clades):
        for c in cl:
            C[c] = C.get(c, 0) + u[k]
        t = frozenset(cl)
        T[t] = T.get(t, 0) + u[k]
        n[t] = n.get(t, 0) + 1
        rep.setdefault(t, k)
    corder = sorted(C, key=lambda c: (-C[c], c))
    torder = sorted(T, key=lambda t: (-T[t], rep[t]))
    tindex = {t: i for i, t in enumerate(torder)}
    mask = (1 << 64) - 1
    return {'clade_bits': np.array([[(c >> (64 * w)) & mask for w in range(W)] for c in corder], dtype=np.uint64).reshape(-1, W),
            'clade_weight': np.array([C[c] for c in corder], dtype=np.uint64),
            'topo_weight': np.array([T[t] for t in torder], dtype=np.uint64),
            'topo_count': np.array([n[t] for t in torder], dtype=np.int32),
            'topo_rep': np.array([rep[t] for t in torder], dtype=np.int32),
            'particle_topo': np.array([tindex[frozenset(cl)] for cl in clades], dtype=np.int32),
            'u': np.array(u, dtype=np.uint64), 'U': U,
            'topo_sets': torder}


def assert_tables_equal(got, exp, what=""):
    for key in ('clade_bits', 'clade_weight', 'topo_weight', 'topo_count', 'topo_rep', 'particle_topo', 'u'):
        np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(exp[key]), err_msg="%s %s" % (what, key))
    assert int(got['U']) == int(exp['U']), what
