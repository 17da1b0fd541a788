"""Restatement in Python of phylo_rell's contract, independent of the library: the counts from
phylo_amd.rng.philox4x32 and the multiply-high rule, the chain with exact rational arithmetic for every fma."""
from fractions import Fraction

import numpy as np

from phylo_amd import rng


def counts(S, b, seed):
    """cnt[s] of replicate b (its global index): draw j is word j & 3 of the block at counter (b, 0, STREAM_BOOT, j >> 2), the
    site (word * S) >> 32 as a 64-bit product."""
    nblk = (S + 3) // 4
    words = np.stack(rng.philox4x32(b, 0, rng.STREAM_BOOT, np.arange(nblk), seed), axis=-1).reshape(-1)[:S]
    sites = [(int(w) * S) >> 32 for w in words]
    return np.bincount(np.array(sites, dtype=np.int64), minlength=S).astype(np.int32)


def fma(a, b, c):
    """round(a * b + c), a, b, c finite doubles: exact in rationals, then int / int, which Python rounds correctly.  An exact zero
    comes out as +0.0, as it does in the chain (it starts at +0.0, and -0.0 + +0.0 = +0.0 to nearest)."""
    e = Fraction(a) * Fraction(b) + Fraction(c)
    return e.numerator / e.denominator


def chain(cnt, x):
    """acc = +0.0; acc = fma(cnt[s], x[s], acc) over ascending s"""
    acc = 0.0
    for c, v in zip(cnt, x):
        acc = fma(float(c), float(v), acc)
    return acc


def rep_loglik(cnt_BxS, x_TxS):
    return np.array([[chain(c, x) for c in cnt_BxS] for x in x_TxS])


def observed(x_TxS):
    return np.array([chain(np.ones(len(x)), x) for x in x_TxS])


def factors(T, S, seed, special=True):
    """test input: exp(U(-30, -1)) with a positive subnormal, 1.0 and a value > 1 among them"""
    r = np.random.default_rng(seed)
    f = np.exp(r.uniform(-30.0, -1.0, size=(T, S)))
    if special:
        flat = f.reshape(-1)
        for k, v in enumerate((5e-324, 1.0, 3.75, 2.2250738585072014e-308 / 8, 1.0 + 2.0 ** -52)):
            flat[(7 * k + 3) % flat.size if flat.size > 5 else k % flat.size] = v
    return f


def first_argmax(R):
    """best[b] by the contract: the lowest t of the greatest R[t][b]"""
    return np.argmax(R, axis=0).astype(np.int32)


# ---- loop restatements of phylo_amd.treetests ----
def tree_tests_loops(obs, R):
    import math
    T, B = len(obs), len(R[0])
    best = max(range(T), key=lambda t: (obs[t], -t))
    out = {'bp': [0.0] * T, 'p_kh': [], 'p_sh': [], 'c_elw': []}
    for b in range(B):
        w = max(range(T), key=lambda t: (R[t][b], -t))
        out['bp'][w] += 1.0 / B
    means = [math.fsum(R[t]) / B for t in range(T)]
    for t in range(T):
        delta = obs[best] - obs[t]
        d = [R[best][b] - R[t][b] for b in range(B)]
        md = math.fsum(d) / B
        out['p_kh'].append(sum(1 for b in range(B) if d[b] - md >= delta) / B)
        n = 0
        for b in range(B):
            M = max(R[u][b] - means[u] for u in range(T))
            n += M - (R[t][b] - means[t]) >= delta
        out['p_sh'].append(n / B)
        acc = 0.0
        for b in range(B):
            m = max(R[u][b] for u in range(T))
            acc += math.exp(R[t][b] - m) / math.fsum(math.exp(R[u][b] - m) for u in range(T))
        out['c_elw'].append(acc / B)
    return {k: np.array(v) for k, v in out.items()}
