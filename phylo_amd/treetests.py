"""Tree-selection statistics from a RELL bootstrap (Context.rell): pure NumPy, no GPU.

Given the observed scores obs[t] of T candidate trees and the replicate scores R[t][b] of B bootstrap replicates
(resampling estimated log-likelihoods, Kishino, Miyata & Hasegawa 1990), with best = argmax obs (lowest index) and
delta_t = obs[best] - obs[t]:

  bp     bootstrap proportion: wins[t] / B, the share of replicates in which t scores highest (ties to the lowest index).
  p_kh   Kishino-Hasegawa test (Kishino & Hasegawa 1989) of t against the best tree, one-sided, centred:
         d_b = R[best][b] - R[t][b];  p = #{b : d_b - mean(d) >= delta_t} / B.
  p_sh   Shimodaira-Hasegawa test (Shimodaira & Hasegawa 1999), which corrects for having picked the best of many trees:
         Rc = R - (row mean);  M_b = max_t Rc[t][b];  p = #{b : M_b - Rc[t][b] >= delta_t} / B.
  c_elw  expected likelihood weight (Strimmer & Rambaut 2002):
         the mean over b of exp(R[t][b] - max_t R[.][b]) / sum_t exp(R[t][b] - max_t R[.][b]).

bp needs the win counts alone; the other three need the replicate matrix (Context.rell(..., want_reps=True)).

  p_au   approximately unbiased test (Shimodaira 2002) of "t is the best tree", from the win counts of a MULTISCALE bootstrap
         (Context.rell_multiscale: replicates of n_k = r_k S sites at K scales): au_scales gives the draws, au_test / au_fit fit
         z_k = -Phi^-1(bp_k) = d / sigma_k + c sigma_k (sigma_k^2 = S / n_k) by weighted least squares; p_au = Phi(c - d).
"""
from __future__ import annotations

from statistics import NormalDist

import numpy as np


def tree_tests(obs, wins, B, reps=None):
    """Per-tree statistics as a dict of [T] arrays: 'bp' always; 'p_kh', 'p_sh', 'c_elw' and 'delta' when reps [T][B] is given."""
    obs = np.asarray(obs, dtype=np.float64).reshape(-1)
    wins = np.asarray(wins, dtype=np.int64).reshape(-1)
    B = int(B)
    T = obs.size
    if wins.shape != (T,) or B < 1:
        raise ValueError("obs and wins must hold one value per tree and B must be >= 1")
    if int(wins.sum()) != B:
        raise ValueError("wins must add up to B (%d != %d)" % (int(wins.sum()), B))
    out = {'bp': wins / float(B)}
    if reps is None:
        return out
    R = np.asarray(reps, dtype=np.float64)
    if R.shape != (T, B):
        raise ValueError("reps must be [T][B] = (%d, %d), got %r" % (T, B, R.shape))
    best = int(np.argmax(obs))
    delta = obs[best] - obs
    d = R[best][None, :] - R
    p_kh = np.count_nonzero(d - d.mean(axis=1, keepdims=True) >= delta[:, None], axis=1) / float(B)
    Rc = R - R.mean(axis=1, keepdims=True)
    p_sh = np.count_nonzero(Rc.max(axis=0)[None, :] - Rc >= delta[:, None], axis=1) / float(B)
    w = np.exp(R - R.max(axis=0)[None, :])
    c_elw = (w / w.sum(axis=0)[None, :]).mean(axis=1)
    out.update(p_kh=p_kh, p_sh=p_sh, c_elw=c_elw, delta=delta, best=best)
    return out


_N01 = NormalDist()
AU_MAX_SCALES, AU_MAX_DRAWS = 64, 65535                 # phylo_rell_multiscale's bounds


def au_ratios(spec):
    """'default' | 'r1,r2,...' -> the list of r (what can be checked before S is known); ValueError on anything else"""
    if str(spec).strip() == 'default':
        return [(5 + i) / 10.0 for i in range(10)]
    try:
        r = [float(x) for x in str(spec).split(',')]
    except ValueError:
        raise ValueError("expected 'default' or a comma list of positive numbers r1,r2,..., got %r" % (spec,))
    if not all(np.isfinite(x) and x > 0 for x in r):
        raise ValueError("every scale r must be a finite number > 0, got %r" % (spec,))
    if len(set(r)) < 2 or len(r) > AU_MAX_SCALES:
        raise ValueError("need 2 .. %d scales, at least two of them distinct, got %r" % (AU_MAX_SCALES, spec))
    return r


def au_scales(S, spec='default'):
    """The scales of the multiscale bootstrap (runner.py --tree_tests_au): 'default' is r = 0.5, 0.6, ..., 1.4 (CONSEL's), otherwise
    a comma list of positive r.  Returns a dict: 'r' [K], 'draws' [K] int32 with draws[k] = max(1, floor(r_k S + 0.5)) sites per
    replicate, and 'sigma2' [K] = S / draws[k] -- from the draws actually made, not from r.  ValueError for anything else, for
    fewer than two distinct draws (the fit has two parameters), more than 64 scales or a draw count above 65535."""
    S = int(S)
    if S < 1:
        raise ValueError("S must be >= 1, got %d" % S)
    r = au_ratios(spec)
    draws = [max(1, int(np.floor(x * S + 0.5))) for x in r]
    if max(draws) > AU_MAX_DRAWS:
        raise ValueError("a replicate draws at most %d sites, r = %g of S = %d asks for %d" % (AU_MAX_DRAWS, r[int(np.argmax(draws))], S, max(draws)))
    if len(set(draws)) < 2:
        raise ValueError("need at least two distinct draw counts, got %r for S = %d" % (draws, S))
    draws = np.array(draws, dtype=np.int32)
    return {'r': np.array(r, dtype=np.float64), 'draws': draws, 'sigma2': S / draws.astype(np.float64)}


def au_fit(bp, sigma2, B):
    """The AU p-value of one hypothesis from its bootstrap proportions bp [K] at the scales sigma2 [K], B replicates each
    (Shimodaira 2002, the weighted least squares fit).  Usable scales are those with 0 < bp < 1; there z_k = -Phi^-1(bp_k) is
    fitted by z_k = d / sigma_k + c sigma_k with weights w_k = B phi(z_k)^2 / (bp_k (1 - bp_k)), the inverse of z_k's variance,
    through the closed 2 x 2 normal equations.  Returns a dict of scalars: 'p_au' = Phi(c - d), 'se_au' = phi(d - c)
    sqrt(V_dd + V_cc - 2 V_dc) with V = (X^T W X)^-1, 'd', 'c', 'rss' (the weighted residual sum of squares, chi^2 with 'df' =
    usable - 2 degrees of freedom under the model), 'au_ok'.  With fewer than two usable scales of distinct sigma2 au_ok is
    False, d, c, se_au are NaN, rss is 0 and p_au is the bp at the scale whose sigma2 is nearest 1."""
    bp = np.asarray(bp, dtype=np.float64).reshape(-1)
    s2 = np.asarray(sigma2, dtype=np.float64).reshape(-1)
    B = int(B)
    if bp.size < 1 or bp.shape != s2.shape or B < 1 or not (s2 > 0).all() or not ((bp >= 0) & (bp <= 1)).all():
        raise ValueError("bp and sigma2 must be [K] with 0 <= bp <= 1 and sigma2 > 0, and B >= 1")
    use = (bp > 0) & (bp < 1)
    n = int(use.sum())
    nan = float('nan')
    if n < 2 or np.unique(s2[use]).size < 2:
        return {'p_au': float(bp[int(np.argmin(np.abs(s2 - 1.0)))]), 'se_au': nan, 'd': nan, 'c': nan, 'rss': 0.0, 'df': n - 2, 'au_ok': False}
    p, sg = bp[use], np.sqrt(s2[use])
    z = np.array([-_N01.inv_cdf(float(v)) for v in p])
    w = B * np.array([_N01.pdf(float(v)) for v in z]) ** 2 / (p * (1.0 - p))
    a, b = 1.0 / sg, sg                                  # the two columns of X
    a11, a12, a22 = np.sum(w * a * a), np.sum(w * a * b), np.sum(w * b * b)
    r1, r2 = np.sum(w * a * z), np.sum(w * b * z)
    det = a11 * a22 - a12 * a12
    d, c = (a22 * r1 - a12 * r2) / det, (a11 * r2 - a12 * r1) / det
    v_dd, v_cc, v_dc = a22 / det, a11 / det, -a12 / det
    res = z - (d * a + c * b)
    return {'p_au': _N01.cdf(float(c - d)), 'se_au': _N01.pdf(float(d - c)) * float(np.sqrt(max(v_dd + v_cc - 2.0 * v_dc, 0.0))),
            'd': float(d), 'c': float(c), 'rss': float(np.sum(w * res * res)), 'df': n - 2, 'au_ok': True}


def au_test(wins, sigma2, B):
    """au_fit for every tree of a multiscale bootstrap: wins [K][T] (Context.rell_multiscale), sigma2 [K] (au_scales), B replicates
    per scale.  Returns a dict of [T] arrays 'p_au', 'se_au', 'd', 'c', 'rss', 'df', 'au_ok', and 'bp' [K][T] = wins / B."""
    wins = np.asarray(wins, dtype=np.int64)
    s2 = np.asarray(sigma2, dtype=np.float64).reshape(-1)
    B = int(B)
    if wins.ndim != 2 or wins.shape[0] != s2.size or B < 1:
        raise ValueError("wins must be [K][T] with one row per scale of sigma2, and B >= 1")
    if (wins < 0).any() or (wins.sum(axis=1) != B).any():
        raise ValueError("every scale's wins must add up to B = %d" % B)
    bp = wins / float(B)
    fits = [au_fit(bp[:, t], s2, B) for t in range(wins.shape[1])]
    out = {k: np.array([f[k] for f in fits]) for k in ('p_au', 'se_au', 'd', 'c', 'rss', 'df', 'au_ok')}
    out['bp'] = bp
    return out


def parse_spec(spec):
    """'B[:SEED]' (runner.py --tree_tests) -> (B, seed); ValueError on anything else.  1 <= B <= 2^20, seed a 64-bit integer >= 0."""
    parts = str(spec).split(':')
    try:
        if len(parts) not in (1, 2):
            raise ValueError
        B, seed = int(parts[0]), int(parts[1]) if len(parts) == 2 else 0
    except ValueError:
        raise ValueError("expected B[:SEED] with integers, got %r" % (spec,))
    if not 1 <= B <= 1 << 20:
        raise ValueError("B must be in 1 .. 2^20, got %d" % B)
    if not 0 <= seed < 1 << 64:
        raise ValueError("SEED must be in 0 .. 2^64 - 1, got %d" % seed)
    return B, seed
