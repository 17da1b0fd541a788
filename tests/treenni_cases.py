"""Shared inputs and bounds of the NNI tests: small trees of every shape, the 50-digit yardstick, E_NNI and
E_EXPL (the restatement's own errors, which set the device tolerances), E_NNI_BIG and E_EXPL_BIG for trees above 128 taxa with the
move sample and the 50-digit log-likelihood that measure them, clade sets, and the 8-taxon search case."""
import numpy as np

import treegrad_ref as TR
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
# Deep trees (N > 128): the restatement's error grows with the depth of the tree -- a move low in a caterpillar sees an outer
# partial that went through hundreds of rounded chains -- and 2.9 does not cover it.  Measured by
# test_treenni_edges_cpu.py::test_reference_against_mpmath_big over all five trees of every case of trees_edges_cases.BIG, the
# first 6 sites of the case's alignment, in the units above: delta over EVERY move (36 870 of them) 18.97 at most
# (caterpillars of 129 / 257 / 512 taxa: 13.34 / 12.76 / 18.97; balanced and random trees: 2.87 to 5.20); the explicit
# comparison over move_sample's 24 moves per tree 1.88 at most (balanced-N257; 1.02 to 1.82 elsewhere).
# test_treenni_edges_cpu.py::test_big_bounds_are_not_stale asserts that the worst of all cases lies above half of each bound.
E_NNI_BIG = 19.0
TOL_NNI_BIG = 8 * E_NNI_BIG * 2.0 ** -53
E_EXPL_BIG = 1.9
TOL_EXPL_BIG = 8 * E_EXPL_BIG * 2.0 ** -53

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


# ---- deep trees (129 to 512 taxa): the move sample of the explicit comparison, the 50-digit log-likelihood of a neighbour -------
def move_sample(child, k=24):
    """At most k moves of one tree, fixed by the tree alone: both entries of the root's row where they exist, of the first and of
    the last row below it, and of the row whose node lies deepest (the first such row); the rest evenly spaced over the other
    entries of nni_moves.  Sorted (row, side) pairs."""
    child = np.asarray(child)
    R = child.shape[0]
    N = R + 1
    moves = nni_moves(child)
    if len(moves) <= k:
        return moves
    depth = np.zeros(R, dtype=np.int64)
    for i in range(R - 1, -1, -1):
        for ch in child[i]:
            if ch >= N:
                depth[ch - N] = depth[i] + 1
    have = set(moves)
    fixed = []
    for r in (R - 1, 0, R - 2, int(np.argmax(depth))):
        fixed += [(r, sd) for sd in range(2) if (r, sd) in have and (r, sd) not in fixed]
    rest = [mv for mv in moves if mv not in fixed]
    at = np.linspace(0, len(rest) - 1, k - len(fixed)).astype(int)
    return sorted(set(fixed) | {rest[i] for i in at})


def matrices_of(b2, blen, M):
    """the branch matrices of lengths b2, every one of which occurs in blen (apply_nni moves lengths, it makes none): M's
    matrices, looked up by length -- what branch_matrices(Q, b2) computes again, without a thousand expm per neighbour"""
    flat = np.asarray(M).reshape(-1, 4, 4)
    by_len = {float(t): flat[i] for i, t in enumerate(np.asarray(blen).reshape(-1))}
    return np.array([by_len[float(t)] for t in np.asarray(b2).reshape(-1)]).reshape(np.shape(b2) + (4, 4))


def mp_loglik(mp, child, M, prior, g, memo):
    """(loglik, sum_s |log L_s|) of one tree at 50 digits by the upward pass alone (site_moves' x, msg and L).  memo, a dict the
    caller keeps per alignment, holds the partial of every subtree met so far under its structure -- a leaf is itself, a node is
    (left subtree, left matrix, right subtree, right matrix) -- so a neighbour costs the nodes above its move and no more."""
    mp.mp.dps = 50
    mpf = mp.mpf
    N, S = g.shape[0], g.shape[1]
    R = N - 1
    ids, xs = memo.setdefault('ids', {}), memo.setdefault('x', {})
    for i in range(N):
        if i not in xs:
            xs[i] = [[mpf(float(v)) for v in g[i, s]] for s in range(S)]
    at = list(range(N)) + [None] * R
    for i in range(R):
        kids = (at[child[i][0]], at[child[i][1]])
        key = (kids[0], M[i, 0].tobytes(), kids[1], M[i, 1].tobytes())
        me = ids.setdefault(key, N + len(ids))
        at[N + i] = me
        if me not in xs:
            Mc = [[[mpf(float(v)) for v in col] for col in M[i, sd].T] for sd in range(2)]      # by columns: (x . M)[j]
            out = []
            for s in range(S):
                m = [[mp.fdot(xs[kids[sd]][s], col) for col in Mc[sd]] for sd in range(2)]
                out.append([m[0][j] * m[1][j] for j in range(4)])
            xs[me] = out
    pm = [mpf(float(v)) for v in prior]
    ll, al = mpf(0), mpf(0)
    for s in range(S):
        L = sum((pm[j] * xs[at[N + R - 1]][s][j] for j in range(4)), mpf(0))
        if L == 0:
            return -mp.inf, mp.inf
        ll += mp.log(L)
        al += abs(mp.log(L))
    return ll, al


def _row_times4(x, M):
    """treegrad_ref._row_times with the four columns of M in one array operation: the same chain per element, the same bits"""
    return TR.fma(x[:, 3:4], M[3], TR.fma(x[:, 2:3], M[2], TR.fma(x[:, 1:2], M[1], x[:, 0:1] * M[0])))


def restated_loglik(child, M, prior, g, memo):
    """treenni_ref.tree_loglik_sites' two numbers and bits, with the partial of every subtree met so far kept in memo as mp_loglik
    keeps it: the neighbours of one tree share all but the nodes above the move"""
    N = g.shape[0]
    R = N - 1
    ids, xs = memo.setdefault('ids', {}), memo.setdefault('x', {})
    at = list(range(N)) + [None] * R
    with np.errstate(all='ignore'):
        for i in range(R):
            kids = (at[child[i][0]], at[child[i][1]])
            key = (kids[0], M[i, 0].tobytes(), kids[1], M[i, 1].tobytes())
            me = ids.setdefault(key, N + len(ids))
            at[N + i] = me
            if me not in xs:
                xk = [g[k] if k < N else xs[k] for k in kids]
                xs[me] = _row_times4(xk[0], M[i, 0]) * _row_times4(xk[1], M[i, 1])
        xr = xs[at[N + R - 1]]
        L = TR.fma(prior[3], xr[:, 3], TR.fma(prior[2], xr[:, 2], TR.fma(prior[1], xr[:, 1], prior[0] * xr[:, 0])))
        lg = np.log(L)
    return float(np.sum(lg)), float(np.sum(np.abs(lg)))


def measure_deep(mp, child, blen, Q, prior, g, sample=None):
    """The restatement against 50 digits on one set of trees, as test_treenni_cpu.py::test_reference_against_mpmath does it:
    (worst error of delta over EVERY move in units of (S + sum_s |d_s|) 2^-53; worst summed error of loglik + delta and of the
    restated log-likelihood of apply_nni's tree against that tree's 50-digit log-likelihood, over move_sample, in units of
    (S + sum_s |log L_s| + sum_s |log L'_s|) 2^-53; moves seen; impossible neighbours among them).  An impossible neighbour must be
    -inf in the restatement, and -inf as an explicit tree too."""
    S = g.shape[1]
    worst_n = worst_x = 0.0
    seen = dead_seen = 0
    for c, b in zip(child, blen):
        memo = {}                                                         # per tree: its subtrees, and those of its neighbours
        M = branch_matrices(Q, b)
        ll, delta, absd = NR.tree_nni(c, M, prior, g)
        ell, eal, emv = mp_tree(mp, c, M, prior, g)
        assert set(emv) == set(nni_moves(c))
        assert np.isnan(delta).sum() == delta.size - len(emv)
        l0, a0 = mp_loglik(mp, c, M, prior, g, memo)
        assert abs(l0 - ell) < mp.mpf(10) ** -40 and abs(a0 - eal) < mp.mpf(10) ** -40
        picked = set(move_sample(c) if sample is None else sample(c))
        rmemo, checked = {}, False
        for (r, sd), (ed, ea, dead) in emv.items():
            seen += 1
            if dead:
                dead_seen += 1
                assert delta[r, sd] == -np.inf, (r, sd)
            else:
                assert np.isfinite(delta[r, sd]), (r, sd)
                assert abs(float(ea) - absd[r, sd]) <= 1e-9 * (1 + absd[r, sd])
                worst_n = max(worst_n, float(abs(mp.mpf(float(delta[r, sd])) - ed) / ((S + ea) * mp.mpf(2) ** -53)))
            if (r, sd) not in picked:
                continue
            c2, b2 = apply_nni(c, b, r, sd)
            M2 = matrices_of(b2, b, M)
            ll2, _ = restated_loglik(c2, M2, prior, g, rmemo)
            if not checked:                                                   # once per tree: the shared partials change no bit
                assert ll2 == NR.tree_loglik_sites(c2, M2, prior, g)[0] or dead
                checked = True
            ell2, eal2 = mp_loglik(mp, c2, M2, prior, g, memo)
            if dead:
                assert ll2 == -np.inf and ell2 == -mp.inf, (r, sd)
                continue
            assert abs(ell2 - (ell + ed)) < mp.mpf(10) ** -40, (r, sd)       # the move IS that tree
            unit = (S + eal + eal2) * mp.mpf(2) ** -53
            both = float((abs(mp.mpf(float(ll + delta[r, sd])) - ell2) + abs(mp.mpf(ll2) - ell2)) / unit)
            worst_x = max(worst_x, both)
    return worst_n, worst_x, seen, dead_seen


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
