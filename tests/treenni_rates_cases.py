"""Shared inputs and bounds of the tests of phylo_trees_nni_rates: the mixtures, E_NNI_RATES and
E_EXPL_RATES (the restatement's own errors against 50 digits, which set the device tolerances), the 50-digit yardstick, the
matrices of every category of every tree, and the 8-taxon search case simulated under Gamma4(0.5)."""
import functools

import numpy as np

import treegrad_rates_ref as GR
import treenni_cases as NC
import treenni_rates_ref as RR
from phylo_amd import rates as R
from treegrad_cases import branch_matrices
from treegrad_rates_cases import MIX_I_G4, category_matrices, simulate_rates
from trees_cases import random_rows

PRIOR = NC.PRIOR

# Measured by test_treenni_rates_cpu.py::test_reference_against_mpmath (every move of treenni_cases.small_cases: N = 3, 4, 5, 8, 12;
# random, caterpillar, balanced; S = 6 with gaps; a GTR-like Q and JC69; under p_inv 0.1 + Gamma4(0.5), under C = 1 and under
# C = 16): the worst |restated delta - 50-digit delta| / ((S + sum_s |d_s|) 2^-53) is 2.86 (C = 1: section 14's figure; +I+G4 1.83;
# C = 16 1.78).  The test asserts that the worst stays at or below E_NNI_RATES and above half of it.
E_NNI_RATES = 2.9
TOL_NNI_RATES = 8 * E_NNI_RATES * 2.0 ** -53     # device against restatement: |difference| <= TOL (S + sum_s |d_s| + |value|)
# The explicit comparison, loglik + delta against the mixture log-likelihood of apply_nni's tree: both sides against the 50-digit
# value of the neighbour, their errors added, in units of (S + sum_s |log m_s| + sum_s |log m'_s|) 2^-53.  Measured by the same
# test: 1.83 (C = 16; +I+G4 1.60; C = 1 1.60, section 14's figure).
E_EXPL_RATES = 1.9
TOL_EXPL_RATES = 8 * E_EXPL_RATES * 2.0 ** -53

MIX_ONE = (np.array([1.0]), np.array([1.0]))
MIX_16 = R.rate_model(0.5, 15, 0.1)                 # +I+G15


def half_half_16():
    """sixteen categories, rate 1 and weight 1/2 at positions 3 and 15, weight 0 and other rates (0 among them) elsewhere: the
    chain gives m = f exactly, so the call must return the one-rate call's bits"""
    rates = np.array([0.0, 0.3, 2.5, 1.0, 0.7, 1.9, 0.05, 4.0, 0.5, 1.5, 3.0, 0.2, 0.9, 1.1, 6.0, 1.0])
    weights = np.zeros(16)
    weights[[3, 15]] = 0.5
    return rates, weights


def tree_category_matrices(Q, blen, rates):
    """[T][C][N-1][2][4][4] for blen [T][N-1][2] and rates [C] or [T][C], by scipy"""
    rates = np.asarray(rates, dtype=np.float64)
    return np.array([category_matrices(Q, b, rates[t] if rates.ndim == 2 else rates) for t, b in enumerate(blen)])


# ---- the 50-digit yardstick ---------------------------------------------------------------------------------------------------------
def mp_tree_rates(mp, child, M, prior, g, weights):
    """one tree at 50 digits, M [C][N-1][2][4][4]: (loglik, sum_s |log m_s|, {move: (delta, sum_s |d_s|, impossible)})"""
    mp.mp.dps = 50
    mpf = mp.mpf
    N, S = g.shape[0], g.shape[1]
    C = len(weights)
    Mm = [[[[[mpf(float(v)) for v in r] for r in M[c, i, sd]] for sd in range(2)] for i in range(N - 1)] for c in range(C)]
    pm = [mpf(float(v)) for v in prior]
    wm = [mpf(float(v)) for v in weights]
    ll, al, mv = mpf(0), mpf(0), {}
    for s in range(S):
        rows = [[mpf(float(v)) for v in g[i, s]] for i in range(N)]
        m, out = RR.site_moves_rates(np.asarray(child).tolist(), Mm, pm, rows, wm, mpf(0))
        ll += mp.log(m)
        al += abs(mp.log(m))
        for key, m2 in out.items():
            d, a, dead = mv.get(key, (mpf(0), mpf(0), False))
            if m2 == 0:
                dead = True
            else:
                d += mp.log(m2 / m)
                a += abs(mp.log(m2 / m))
            mv[key] = (d, a, dead)
    return ll, al, mv


def mp_loglik_rates(mp, child, M, prior, g, weights, memo):
    """(mixture loglik, sum_s |log m_s|) of one tree at 50 digits by the upward pass of every category alone.  memo, a dict the
    caller keeps per alignment and mixture, holds the partial of every subtree met so far under (category, structure) -- a leaf is
    itself, a node is (left subtree, left matrix, right subtree, right matrix) -- so a neighbour costs the nodes above its move"""
    mp.mp.dps = 50
    mpf = mp.mpf
    N, S = g.shape[0], g.shape[1]
    R_ = N - 1
    pm = [mpf(float(v)) for v in prior]
    m = [mpf(0)] * S
    for c in range(len(weights)):
        ids, xs = memo.setdefault(('ids', c), {}), memo.setdefault(('x', c), {})
        for i in range(N):
            if i not in xs:
                xs[i] = [[mpf(float(v)) for v in g[i, s]] for s in range(S)]
        at = list(range(N)) + [None] * R_
        for i in range(R_):
            kids = (at[child[i][0]], at[child[i][1]])
            key = (kids[0], M[c, i, 0].tobytes(), kids[1], M[c, i, 1].tobytes())
            me = ids.setdefault(key, N + len(ids))
            at[N + i] = me
            if me not in xs:
                Mc = [[[mpf(float(v)) for v in col] for col in M[c, i, sd].T] for sd in range(2)]
                out = []
                for s in range(S):
                    e = [[mp.fdot(xs[kids[sd]][s], col) for col in Mc[sd]] for sd in range(2)]
                    out.append([e[0][j] * e[1][j] for j in range(4)])
                xs[me] = out
        w = mpf(float(weights[c]))
        for s in range(S):
            m[s] += w * mp.fdot(pm, xs[at[N + R_ - 1]][s])
    ll, al = mpf(0), mpf(0)
    for s in range(S):
        if m[s] == 0:
            return -mp.inf, mp.inf
        ll += mp.log(m[s])
        al += abs(mp.log(m[s]))
    return ll, al


# ---- the search case: an alignment simulated under Gamma4(0.5) along an 8-taxon tree; that tree and trees one, two, three NNIs away ---
# Seed and S chosen by test_treenni_rates_cpu.py::test_nni_search_under_rates' margins.  SEARCH_LO, the lower bound the search's
# climbs keep every length above (optimize_branches' lo), is part of the case: at a wrong topology the branch that contradicts the
# data climbs to its bound, and at the default bound of 1e-8 the three resolutions round a branch that short have one
# likelihood -- both of its moves have |delta| ~ 1e-7, on either side of eps by luck (measured over 76 seeds and sizes: no case had
# its decisions clear of 10 eps).  At 1e-3 the resolutions differ by about 1e-3 times a gradient, far from eps = 1e-6.
SEARCH_SEED, SEARCH_S, SEARCH_EXTRA, SEARCH_LO = 2, 400, 0.05, 1e-3     # (EXTRA: added to every length of the generating tree)
SEARCH_MIX = R.rate_model(0.5, 4)


@functools.lru_cache(maxsize=None)
def search_case(seed=SEARCH_SEED, S=SEARCH_S, extra=SEARCH_EXTRA):
    """(leaves, Q, prior, child [4][7][2], blen [4][7][2], the generating tree's rows)"""
    from treenni_cases import clades
    from phylo_amd.treesearch import apply_nni, nni_moves
    N = 8
    rng = np.random.default_rng(seed)
    Q = NC.gtr_Q()
    c0, b0 = random_rows(N, rng, zeros=False)
    b0 = b0 + extra
    g = simulate_rates(c0, b0, Q, PRIOR, S, rng, *SEARCH_MIX)
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
    return g, Q, PRIOR, np.array(child), np.array(blen), c0


def reference_fns(g, Q, prior, rates, weights):
    """grad_fn and nni_fn of nni_search over the restatements under one mixture (scipy's expm; the mixing chain by fma over arrays)"""
    def grad_fn(child, b):
        res = [GR.tree_grad_rates(c, category_matrices(Q, x, rates), Q, prior, g, x, rates, weights, exact_mix=False) for c, x in zip(child, b)]
        return tuple(np.array([r[k] for r in res]) for k in ('loglik', 'grad', 'curv'))

    def nni_fn(child, b):
        ll, delta, _ = RR.trees_nni_rates(child, tree_category_matrices(Q, b, rates), prior, g, rates, weights, exact_mix=False)
        return ll, delta

    return grad_fn, nni_fn
