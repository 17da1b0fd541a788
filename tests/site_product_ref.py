"""Plain restatements of the site-product contract for the tests: the per-factor update of a running product
kept as a mantissa in [1,2) and an integer exponent, the inputs that walk its edges, which branch of the pair form a triple takes,
the canonical column layout of a row, and the exact value of a sum of logs.  Nothing here shares code with the library or the C
oracle: math.frexp / numpy.frexp, IEEE binary64 products (Python floats), Python integers, fractions and mpmath -- except that the
log of a factor that is not a positive normal number is a function the CALLER supplies (the tests pass the oracle's log, and hold
it within an ulp of mpmath on its own)."""
import math
from fractions import Fraction

import mpmath as mp
import numpy as np

U = 2.0 ** -53                                   # unit roundoff of binary64
TINY = 2.0 ** -1022                              # smallest positive normal number
KEEP_MIN = 2.0 ** -1021                          # the pair form keeps q in [2^-1021, inf)
MAXF = float(np.finfo(np.float64).max)
SUBMAX = float(np.nextafter(TINY, 0.0))          # largest subnormal
BRANCHES = ('kept', 'x1', 'x2', 'small', 'inf')  # pair kept; rejected for x1; for x2; for q < 2^-1021; for q = inf

GRID_X = [2.0 ** -1074, 2.0 ** -1023, SUBMAX, TINY, TINY * (1 + 2.0 ** -52), 2.0 ** -511, 2.0 ** -510, 1 - 2.0 ** -53, 1.0,
          1 + 2.0 ** -52, 2.0 ** 511, 2.0 ** 512, MAXF, math.inf, math.nan, 0.0, -0.0, -1.0, -math.inf]
GRID_P = [1.0, 1 + 2.0 ** -52, 1.5, 2 - 2.0 ** -52]


def positive_normal(x):
    return TINY <= x <= MAXF                     # False for NaN, zeros, subnormals, negatives and +inf


def lp_mul(state, x, log):
    """One factor into (p, E, extra).  `log` is called for factors that are not positive normal numbers only."""
    p, E, extra = state
    if not positive_normal(x):
        return p, E, extra + log(x)
    m, e = math.frexp(x)                         # x = m 2^e, m in [0.5, 1)
    p = p * (2.0 * m)                            # ONE rounding; [1, 4)
    E += e - 1
    if p >= 2.0:
        p, E = 0.5 * p, E + 1                    # exact
    return p, E, extra


def lp_two(p, x1, x2, log):
    """The contract's statement of a pair: two per-factor updates from a fresh (p, 0, 0.0)."""
    return lp_mul(lp_mul((p, 0, 0.0), x1, log), x2, log)


def lp_two_np(p, x1, x2, log):
    """lp_two on arrays (numpy.frexp, float64 products); log: array -> array, called on the factors that are not positive normal"""
    p = np.array(p, dtype=np.float64)
    E = np.zeros(p.shape, dtype=np.int64)
    extra = np.zeros(p.shape)
    with np.errstate(all='ignore'):
        for x in (np.asarray(x1, dtype=np.float64), np.asarray(x2, dtype=np.float64)):
            ok = (x >= TINY) & (x <= MAXF)
            m, e = np.frexp(np.where(ok, x, 1.0))
            q = p * (2.0 * m)
            up = q >= 2.0
            p = np.where(ok, np.where(up, 0.5 * q, q), p)
            E = E + np.where(ok, e - 1 + up, 0)
            lg = np.zeros(p.shape)
            if (~ok).any():
                lg[~ok] = log(x[~ok])
            extra = np.where(ok, extra, extra + lg)
    return p, E, extra


def branch_of(p, x1, x2):
    """Index into BRANCHES of every triple, from the inputs alone: the pair form's product is (p x1) x2 in binary64."""
    p, x1, x2 = (np.asarray(a, dtype=np.float64) for a in (p, x1, x2))
    ok1 = (x1 >= TINY) & (x1 <= MAXF)
    ok2 = (x2 >= TINY) & (x2 <= MAXF)
    with np.errstate(all='ignore'):
        q = (p * x1) * x2
    out = np.zeros(p.shape, dtype=np.int64)
    out[ok1 & ok2 & np.isinf(q)] = 4
    out[ok1 & ok2 & (q < KEEP_MIN)] = 3
    out[ok1 & ~ok2] = 2
    out[~ok1] = 1
    return out


def boundary_grid():
    """every p of GRID_P with every ordered pair of GRID_X"""
    P, X1, X2 = np.meshgrid(GRID_P, GRID_X, GRID_X, indexing='ij')
    return P.ravel(), X1.ravel(), X2.ravel()


def steered_triples(n_mantissas=400, seed=5):
    """Triples whose product (p x1) x2 lands on 2^-1022, 2^-1021 or 2^1024, a few ulps below or above: m2 within three ulps of
    2 / m1 puts the mantissa product m1 m2 on 2 or beside it, inexact products included (the ones that ROUND onto the boundary),
    and the exponents move that 2 to the boundary.  The running value carries m1 in half of them, x1 in the other half.
    Returns p, x1, x2 and `target`, the boundary's exponent."""
    rng = np.random.default_rng(seed)
    m1 = np.concatenate([[1.5, 1.25, 1.75, 1 + 2.0 ** -52, 2 - 2.0 ** -52], 1.0 + rng.random(n_mantissas)])
    ps, x1s, x2s, tg = [], [], [], []
    for target in (-1022, -1021, 1024):
        for k in range(-3, 4):
            m2 = 2.0 / m1
            for _ in range(abs(k)):
                m2 = np.nextafter(m2, 4.0 if k > 0 else 0.0)
            m2 = np.clip(m2, 1.0, 2 - 2.0 ** -52)
            a = rng.integers(-900, -100, m1.size) if target < 0 else rng.integers(100, 900, m1.size)   # b normal too
            b = (target - 1) - a                                  # m1 m2 ~ 2: (p x1) x2 ~ 2^(a + b + 1) = 2^target
            half = np.arange(m1.size) % 2 == 0
            ps.append(np.where(half, m1, 1.0))
            x1s.append(np.where(half, np.ldexp(1.0, a), np.ldexp(m1, a)))
            x2s.append(np.ldexp(m2, b))
            tg.append(np.full(m1.size, target))
        a0 = -300 if target < 0 else 500                          # and the boundary itself, exactly: powers of two
        ps.append(np.array([1.0])); x1s.append(np.array([2.0 ** a0])); x2s.append(np.array([2.0 ** (target - a0)]))
        tg.append(np.array([target]))
    return tuple(np.concatenate(v) for v in (ps, x1s, x2s, tg))


def exact_product(p, x1, x2):
    return Fraction(float(p)) * Fraction(float(x1)) * Fraction(float(x2))


def random_triples(n, seed):
    """p uniform in [1,2); factors from every class: exponents over the whole normal range, around +-511 (so that pairs leave the
    range together), subnormals, and a sprinkle of 0, -0, +-inf, NaN and negative numbers"""
    rng = np.random.default_rng(seed)
    p = np.clip(1.0 + rng.random(n), 1.0, 2 - 2.0 ** -52)

    def factors():
        kind = rng.integers(0, 10, n)
        m = 1.0 + rng.random(n)
        e = np.where(kind < 3, rng.integers(-1022, 1024, n),
                     np.where(kind < 5, rng.integers(-530, -490, n),
                              np.where(kind < 7, rng.integers(490, 530, n), rng.integers(-40, 40, n))))
        x = np.ldexp(m, e)
        sub = kind == 7
        x[sub] = np.ldexp(m[sub], rng.integers(-1074, -1022, int(sub.sum())))
        spec = kind == 8
        x[spec] = rng.choice([0.0, -0.0, math.inf, -math.inf, math.nan, -1.0, -3e-310, 5e-324, -2.5e300], int(spec.sum()))
        return x
    return p, factors(), factors()


# ---- the canonical layout of a row's sum (contract v5) and its exact value -------------------------------------------------------

def columns_of(S, T):
    """[(tile, column, [sites in increasing order])] for the non-empty columns of a row of S sites under site tile T"""
    out = []
    for tile, s0 in enumerate(range(0, S, T)):
        s1 = min(s0 + T, S)
        for c in range(min(64, s1 - s0)):
            out.append((tile, c, list(range(s0 + c, s1, 64))))
    return out


def exact_log_sum(f, dps=60):
    """sum of log f_s at `dps` digits; f: finite positive doubles"""
    with mp.workdps(dps):
        tot = mp.mpf(0)
        for v in f:
            tot += mp.log(mp.mpf(float(v)))
        return tot


def row_bound(f, T, dps=60):
    """(exact sum of logs, error bound of the contract's evaluation) for a row of finite positive factors f under site tile T:
    u (S + a) + u sum_c w_c, a = 4 * (non-empty columns) + 1, b = 3 + 6 + (tiles - 1); w_c = b |v_c| for a column of normal factors,
    (b + 2 + m_c) sum_s |log f_s| for a column with m_c > 0 subnormal ones; the derivation is in tests/test_site_product_host.py."""
    S = len(f)
    tiles = (S + T - 1) // T
    cols = columns_of(S, T)
    a = 4 * len(cols) + 1
    b = 3 + 6 + (tiles - 1)
    with mp.workdps(dps):
        total, weighted = mp.mpf(0), mp.mpf(0)
        for _, _, sites in cols:
            v, av = mp.mpf(0), mp.mpf(0)
            m_c = 0
            for s in sites:
                lg = mp.log(mp.mpf(float(f[s])))
                v += lg
                av += abs(lg)
                m_c += 0.0 < f[s] < TINY
            total += v
            weighted += (b + 2 + m_c) * av if m_c else b * abs(v)
        return total, float(U * (S + a) + U * weighted)
