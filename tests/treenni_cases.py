"""Shared inputs and bounds of the NNI tests: small trees of every shape, the 50-digit yardstick, E_NNI and
E_EXPL (the restatement's own errors, which set the device tolerances), clade sets, and the 8-taxon search case."""
import numpy as np

import treenni_ref as NR
from oracle import cpu_ref as O
from phylo_amd.treesearch import apply_nni, nni_moves
from treegrad_cases import branch_matrices, simulate
from trees_cases import balanced_rows, caterpillar_rows, random_rows

PRIOR = np.array([0.1, 0.2, 0.3, 0.4])

# Measured by test_treenni_cpu.py::test_reference_against_mpmath (N = 3, 4, 5, 8, 12; random, caterpillar, balanced; S = 6 with
# gaps; a GTR-like Q and JC69; every move): the worst |restated delta - 50-digit delta| / ((S + sum_s |d_s|) 2^-53) is 2.86; the
# test asserts that it stays at or below E_NNI and above half of it.
E_NNI = 2.9
TOL_NNI = 8 * E_NNI * 2.0 ** -53       # device against restatement: |difference| <= TOL_NNI (S + sum_s |d_s| + |value|)
# The explicit comparison, loglik + delta against the log-likelihood of apply_nni's tree: both sides against the 50-digit
# log-likelihood of the neighbour, their errors added, in units of (S + sum_s |log L_s| + sum_s |log L'_s|) 2^-53 (the sums over
# the tree and over the neighbour).  Measured by the same test: 1.60.
E_EXPL = 1.7
TOL_EXPL = 8 * E_EXPL * 2.0 ** -53     # device: |(loglik + delta) - loglik of the neighbour| <= TOL_EXPL (S + sum |log L| + sum |log L'|)

SHAPES = {'random': lambda n, rng: random_rows(n, rng, zeros=False), 'caterpillar': caterpillar_rows, 'balanced': balanced_rows}


def gtr_Q(seed=7):
    return O.get_Q(np.random.default_rng(seed).normal(size=(4, 4)))


def gapped(N, S, rng):
    codes = rng.integers(0, 5, size=(N, S))
    return np.stack([(codes == b) | (codes == 4) for b in range(4)], axis=-1).astype(np.float64)


def small_cases():
    """(name, child, blen, Q, leaves) over N = 3, 4, 5, 8, 12, the three shapes, GTR-like and JC69, S = 6 with gaps"""
    out = []
    for N in (3, 4, 5, 8, 12):
        for shape, make in SHAPES.items():
            for jc in (False, True):
                rng = np.random.default_rng(1000 * N + 10 * len(shape) + jc)
                child, blen = make(N, rng)
                Q = O.jc_Q() if jc else O.get_Q(rng.normal(size=(4, 4)))
                out.append(("N%d-%s-%s" % (N, shape, 'jc' if jc else 'gtr'), child, blen, Q, gapped(N, 6, rng)))
    return out


def rooted_shapes(N):
    """every rooted shape of N = 3 or 4 leaves as rows, a root with a leaf child on either side included"""
    if N == 3:
        return [np.array(c, dtype=np.int32) for c in ([[0, 1], [3, 2]], [[1, 2], [0, 3]])]
    return [np.array(c, dtype=np.int32) for c in ([[0, 1], [2, 3], [4, 5]], [[0, 1], [4, 2], [5, 3]], [[0, 1], [2, 4], [3, 5]],
                                                    [[2, 3], [1, 4], [0, 5]])]


def clades(child):
    """the unrooted bipartitions of a tree in rows: for every internal edge the side without leaf 0, as a frozenset (sides of one
    or N-1 leaves dropped; the two edges at the root are one edge)"""
    child = np.asarray(child)
    R = child.shape[0]
    N = R + 1
    below = [frozenset([i]) for i in range(N)] + [None] * R
    for i in range(R):
        below[N + i] = below[child[i, 0]] | below[child[i, 1]]
    every = below[N + R - 1]
    out = set()
    for i in range(R - 1):
        s = below[N + i]
        s = every - s if 0 in s else s
        if 1 < len(s) < N - 1:
            out.add(s)
    return out


def mp_tree(mp, child, M, prior, g):
    """one tree at 50 digits: (loglik, sum_s |log L_s|, {move: (delta, sum_s |d_s|, impossible)})"""
    mp.mp.dps = 50
    mpf = mp.mpf
    N, S = g.shape[0], g.shape[1]
    Mm = [[[[mpf(float(v)) for v in r] for r in M[i, sd]] for sd in range(2)] for i in range(N - 1)]
    pm = [mpf(float(v)) for v in prior]
    ll, al, mv = mpf(0), mpf(0), {}
    for s in range(S):
        rows = [[mpf(float(v)) for v in g[i, s]] for i in range(N)]
        L, out = NR.site_moves(np.asarray(child).tolist(), Mm, pm, rows, mpf(0))
        ll += mp.log(L)
        al += abs(mp.log(L))
        for key, Lp in out.items():
            d, a, dead = mv.get(key, (mpf(0), mpf(0), False))
            if Lp == 0:
                dead = True
            else:
                d += mp.log(Lp / L)
                a += abs(mp.log(Lp / L))
            mv[key] = (d, a, dead)
    return ll, al, mv


# ---- the search case: an alignment simulated along an 8-taxon tree; that tree and trees one, two and three NNIs away ------------
SEARCH_SEED, SEARCH_S, SEARCH_JC = 20, 300, False      # chosen by test_treenni_cpu.py::test_nni_search's margins


def search_case(seed=SEARCH_SEED, S=SEARCH_S, jc=SEARCH_JC):
    """(leaves, Q, prior, child [4][7][2], blen [4][7][2], the generating tree's rows)"""
    N = 8
    rng = np.random.default_rng(seed)
    Q = O.jc_Q() if jc else gtr_Q()
    prior = np.full(4, 0.25) if jc else PRIOR
    c0, b0 = random_rows(N, rng, zeros=False)
    b0 = b0 + 0.05
    g = simulate(c0, b0, Q, prior, S, rng)
    child, blen = [c0], [b0]
    c, b = c0, b0
    for _ in range(3):
        for _ in range(100):                                # a move that takes the tree one step further from the generating tree
            mv = nni_moves(c)[rng.integers(0, len(nni_moves(c)))]
            c2, b2 = apply_nni(c, b, *mv)
            if len(clades(c2) - clades(c0)) == len(clades(c) - clades(c0)) + 1:
                break
        else:
            raise AssertionError("no move leads away")
        c, b = c2, b2
        child.append(c)
        blen.append(b)
    return g, Q, prior, np.array(child), np.array(blen), c0


def reference_fns(g, Q, prior):
    """grad_fn and nni_fn of nni_search over the restatements (scipy's expm)"""
    import treegrad_ref as TR

    def grad_fn(child, b):
        ll, grad, curv, _ = TR.trees_grad(child, branch_matrices(Q, b), Q, prior, g)
        return ll, grad, curv

    def nni_fn(child, b):
        ll, delta, _ = NR.trees_nni(child, branch_matrices(Q, b), prior, g)
        return ll, delta

    return grad_fn, nni_fn
