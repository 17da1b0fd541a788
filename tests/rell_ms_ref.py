"""Restatement in Python of phylo_rell_multiscale's contract on top of tests/rell_ref.py, independent of
the library: the counts of replicate b of scale k, the exact-rational chain, the lexicographic best."""
import numpy as np

import rell_ref
from phylo_amd import rng


def counts(S, draws, k, b, seed):
    """cnt[s] of replicate b of scale k: draws[k] draws, draw j word j & 3 of the block at counter (b, k, STREAM_BOOT, j >> 2), the
    site (word * S) >> 32 as a 64-bit product"""
    nd = int(draws[k])
    words = np.stack(rng.philox4x32(b, k, rng.STREAM_BOOT, np.arange((nd + 3) // 4), seed), axis=-1).reshape(-1)[:nd]
    sites = [(int(w) * S) >> 32 for w in words]
    return np.bincount(np.array(sites, dtype=np.int64), minlength=S).astype(np.int32)


def best_lex(R):
    """best[b]: the t of the lexicographic maximum of (R[t][b], -t)"""
    R = np.asarray(R)
    return np.array([max(range(R.shape[0]), key=lambda t: (R[t, b], -t)) for b in range(R.shape[1])], dtype=np.int32)


def rep_loglik(cnt_BxS, x_TxS):
    return rell_ref.rep_loglik(cnt_BxS, x_TxS)


def host(f, draws, B, seed, hook, **kw):
    """every scale of the library's host loop, stacked: counts [K][B][S], rep_loglik [K][T][B], best [K][B]"""
    outs = [hook(f, draws, k, 0, B, seed, **kw) for k in range(len(draws))]
    return {key: np.stack([o[key] for o in outs]) for key in ('counts', 'rep_loglik', 'best')}
