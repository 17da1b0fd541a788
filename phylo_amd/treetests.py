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
"""
from __future__ import annotations

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
