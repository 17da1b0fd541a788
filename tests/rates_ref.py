"""Plain restatements of the rate-mixture contract of phylo_trees_loglik_rates for the tests: no library
code, exact rational arithmetic rounded once."""
from fractions import Fraction

import numpy as np


def fma(a, b, c):
    """a * b + c rounded once: the sum is exact as a Fraction, and float() of a Fraction is correctly rounded"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def mix(weights, factors):
    """The site values of the contract: factors [C][...] of the categories, weights [C].  m = weights[0] * f_0 (one rounding),
    then m = fma(weights[c], f_c, m) for c = 1 .. C-1 in ascending order.  Finite inputs."""
    w = [float(x) for x in np.asarray(weights, dtype=np.float64).reshape(-1)]
    f = np.asarray(factors, dtype=np.float64)
    assert f.shape[0] == len(w) >= 1
    flat = f.reshape(len(w), -1)
    out = np.empty(flat.shape[1])
    for s in range(flat.shape[1]):
        m = w[0] * float(flat[0, s])
        for c in range(1, len(w)):
            m = fma(w[c], float(flat[c, s]), m)
        out[s] = m
    return out.reshape(f.shape[1:])
