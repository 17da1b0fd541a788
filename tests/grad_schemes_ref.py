"""Inputs and references for tests/test_gpu_grad_schemes.py (TEST INFRASTRUCTURE ONLY): the pairs (A, E) on which the reverse pass's
Frechet series (pg_expm4_frechet / pg_expm4_frechet_row, phylo_amd/csrc/phylo_grad.h) is probed, the scaling and term class the
series picks for each of them (restated here to lay the batches out, not to compute anything), and the two references:
  A  mpmath at 60 digits: the upper-right block of exp([[A, E], [0, A]]) by scaling with 2^-k, Taylor and k squarings;
  B  scipy.linalg.expm_frechet, which a host-only test of that file pins against A on A's grid.
No GPU and no library of the project is used here."""
import os

import numpy as np

from oracle import cpu_ref as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

THETA_CLASSES = (0.01, 0.05, 0.15, 0.3, 0.5)                # the series' class boundaries of theta = ||A||_1 2^-s
NTERMS = (8, 10, 13, 15, 18)
S_MAX = 12                                                  # ||A||_1 <= 4096 = 0.5 * 2^13: s = 0 .. 13 (13 at the very top only)


def generators():
    """Row-normalised Q of get_Q(y) at spread 0, 0.3 and 3.0, and the JC and GTR-init matrices of the golden expm tables."""
    rng = np.random.default_rng(2024)
    ex = np.load(os.path.join(GOLDEN, "expm_tables.npz"))
    out = [("spread%g" % sp, O.get_Q(rng.normal(size=(4, 4)) * sp)) for sp in (0.0, 0.3, 3.0)]
    return out + [("jc", ex["Q/jc"]), ("gtr_init", ex["Q/gtr_init"])]


def a_of(Q, b):
    """A = (Q b)^T as pg_node_finish and pg_twist_finish form it: At[i][j] = Q[j][i] * b."""
    return np.ascontiguousarray((np.asarray(Q, dtype=np.float64) * np.float64(b)).T)


def norm1_device(A):
    """||A||_1 with the device's order of additions (column sums from +0.0, rows 0..3), for [n, 4, 4]."""
    a = np.abs(np.asarray(A, dtype=np.float64).reshape(-1, 4, 4))
    cs = np.zeros((a.shape[0], 4))
    for i in range(4):
        cs = cs + a[:, i, :]
    return cs.max(axis=1)


def plan(A):
    """(s, nterms) the series picks: s doublings of lim = 0.5 until norm <= lim (at most 60), the class from theta = norm 2^-s."""
    norm = norm1_device(A)
    s = np.zeros(norm.shape, dtype=np.int64)
    lim = np.full(norm.shape, 0.5)
    for _ in range(60):
        more = norm > lim
        if not more.any():
            break
        lim = np.where(more, lim * 2.0, lim)
        s += more
    theta = norm * np.ldexp(1.0, -s)
    nt = np.full(norm.shape, NTERMS[-1], dtype=np.int64)
    for bound, n in reversed(list(zip(THETA_CLASSES[:-1], NTERMS[:-1]))):
        nt = np.where(theta <= bound, n, nt)
    return s, nt


def edge_b(Q, target):
    """Adjacent doubles (b_lo, b_hi) with ||A(b_lo)||_1 <= target < ||A(b_hi)||_1: a boundary approached by one ulp of b."""
    nq = norm1_device(a_of(Q, 1.0))[0]
    b = np.float64(target) / nq
    for _ in range(64):
        if norm1_device(a_of(Q, b))[0] <= target:
            break
        b = np.nextafter(b, 0.0)
    for _ in range(64):
        up = np.nextafter(b, np.inf)
        if norm1_device(a_of(Q, up))[0] > target:
            return float(b), float(up)
        b = up
    raise AssertionError("no boundary found near %r" % target)


def edge_bs(Q, scales):
    """b = 0, 1e-300, 1e-8; every class boundary of theta at the scalings in `scales` (0.5 2^s is the scaling boundary itself),
    from both sides."""
    bs = [0.0, 1e-300, 1e-8]
    for s in scales:
        for th in THETA_CLASSES if s == 0 else THETA_CLASSES[3:]:       # (for s >= 1 theta > 0.25: only 0.3 and 0.5 are met)
            bs.extend(edge_b(Q, np.ldexp(th, s)))
    return bs


def special_E(rng, kind):
    E = rng.normal(size=(4, 4))
    if kind == 1:
        E[:] = 0.0
    elif kind == 2:
        E[:] = 0.0
        E[rng.integers(0, 4), rng.integers(0, 4)] = rng.normal()
    elif kind == 3:
        E *= 1e-150
    elif kind == 4:
        E *= 1e150
    return E


def grid_A():
    """Reference A's grid: about 300 pairs.  Every generator at every edge b of s = 0, 1, 2, 3, 6, 12 and the scaling boundary of
    every s, plus log-uniform b up to ||A||_1 = 4096; E random normal, every fifth pair one of the special E in turn."""
    rng = np.random.default_rng(7)
    As, Es, tags = [], [], []
    for name, Q in generators():
        nq = norm1_device(a_of(Q, 1.0))[0]
        bs = edge_bs(Q, (0, 1, 2, 3, 6, 12))
        for s in (4, 5, 7, 8, 9, 10, 11):
            bs.extend(edge_b(Q, np.ldexp(0.5, s)))
        bs.extend(np.exp(rng.uniform(np.log(1e-6), np.log(4096.0 / nq), 10)))
        bs.append(edge_b(Q, 4096.0)[0])
        for b in bs:
            As.append(a_of(Q, b))
            Es.append(special_E(rng, 1 + (len(As) // 5) % 4 if len(As) % 5 == 0 else 0))
            tags.append((name, float(b)))
    return np.array(As), np.array(Es), tags


def batch_B(n=20037):
    """Reference B's batch: the grid of A, every generator at every edge b of every s = 0 .. 12, and log-uniform b over
    ||A||_1 in [1e-9, 4096] for the rest; n is neither a multiple of 64 (a wave of form 0) nor of 4 * 64 (form 1's workgroup is
    64 matrices: 4 n is not a multiple of 256)."""
    assert n % 64 and (4 * n) % 256
    rng = np.random.default_rng(8)
    A0, E0, _ = grid_A()
    As, Es = list(A0), list(E0)
    gens = generators()
    for name, Q in gens:
        for b in edge_bs(Q, range(S_MAX + 1)):
            As.append(a_of(Q, b))
            Es.append(special_E(rng, int(rng.integers(0, 5))))
    while len(As) < n:
        name, Q = gens[len(As) % len(gens)]
        nq = norm1_device(a_of(Q, 1.0))[0]
        lo, hi = (1e-9, 1e-3) if rng.integers(0, 10) == 0 else (1e-3, 4096.0)   # (s = 0 for under half of the batch: see shuffled_layout)
        As.append(a_of(Q, np.exp(rng.uniform(np.log(lo), np.log(hi))) / nq))
        Es.append(special_E(rng, int(rng.integers(1, 5)) if rng.integers(0, 16) == 0 else 0))
    A, E = np.array(As[:n]), np.array(Es[:n])
    assert norm1_device(A).max() <= 4096.0
    return A, E


def shuffled_layout(s, nt, seed=9):
    """A permutation under which neighbours differ in s wherever a partner is left, and in the term class when they can (for
    s >= 1 only the classes 15 and 18 occur): random, then a greedy pass that swaps a clashing element with a later one."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(s))
    for i in range(1, len(perm)):
        p = perm[i - 1]
        if s[perm[i]] != s[p] and nt[perm[i]] != nt[p]:
            continue
        best = -1
        for j in range(i + 1, min(i + 200, len(perm))):
            if s[perm[j]] != s[p]:
                if nt[perm[j]] != nt[p]:
                    best = j
                    break
                if best < 0:
                    best = j
        if best >= 0 and (s[perm[i]] == s[p] or nt[perm[best]] != nt[p]):
            perm[i], perm[best] = perm[best], perm[i]
    return perm


def frechet_mpmath(A, E, digits=60, k=12):
    """Reference A for one pair: exp([[A, E], [0, A]]) by 2^-k scaling, Taylor to below 10^-digits and k squarings, carried out on
    the blocks (X, D) -- the block matrix stays block triangular -- at `digits` decimal digits; returns L as float64."""
    import mpmath as mp
    with mp.workdps(digits):
        Am = mp.matrix(A.tolist()) * mp.mpf(2) ** (-k)
        Em = mp.matrix(E.tolist()) * mp.mpf(2) ** (-k)
        X, D = mp.eye(4), mp.zeros(4)
        SX, SD = mp.eye(4), mp.zeros(4)
        na = max(mp.norm(Am, 1), mp.mpf(10) ** (-400))
        tol = mp.mpf(10) ** (-(digits + 5))
        term = mp.mpf(1)
        for j in range(1, 200):
            D = (X * Em + D * Am) / j
            X = (X * Am) / j
            SX += X
            SD += D
            term = term * na / j
            if term < tol and j > 2:
                break
        for _ in range(k):
            SD = SX * SD + SD * SX
            SX = SX * SX
        return np.array([[float(SD[i, j]) for j in range(4)] for i in range(4)])


def frechet_scipy(A, E):
    """Reference B: scipy.linalg.expm_frechet per pair, [n, 4, 4]."""
    from scipy.linalg import expm_frechet
    out = np.empty_like(A)
    for i in range(A.shape[0]):
        out[i] = expm_frechet(A[i], E[i], compute_expm=False, check_finite=False)
    return out


def rel_err(L, ref):
    """max |L - ref| / max |ref| per matrix; 0 where both vanish identically (E = 0)."""
    num = np.max(np.abs(L - ref), axis=(1, 2))
    den = np.max(np.abs(ref), axis=(1, 2))
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))
