"""Shared numbers of the ancestral-state tests: E_REF_ANC, the worst error of the NumPy restatement
(treeanc_ref.py) against the same formulas at 50 digits, which sets the device tolerance, and the restatement's worst row sum."""
import numpy as np

# Measured by test_treeanc_cpu.py::test_reference_against_mpmath (N = 5, S = 8, gaps, 20 trees, GTR-like and JC69) before the kernel
# ran: the worst |reference - 50-digit value| / (|value| 2^-53) over every posterior is 7.17.  The unit is the value itself: every
# term of a posterior is non-negative, nothing cancels.  The test asserts that it stays at or below E_REF_ANC.
E_REF_ANC = 7.2
TOL_ANC = 8 * E_REF_ANC * 2.0 ** -53          # device against reference: |difference| <= TOL_ANC |reference| (section 13's factor)
TINY = 2.0 ** -900                            # below this a posterior is held to TOL_ANC * TINY absolute
# Measured there too: the worst |sum_j post_j - 1| of the restatement is 6 * 2^-53 (post is not renormalised); held at 8 times that.
SUM_ERR = 6 * 2.0 ** -53
SUM_TOL = 8 * SUM_ERR


PRIOR = np.array([0.1, 0.2, 0.3, 0.4])
T = 37
MAX_EXCLUDED = 0.01                           # the share of node-sites per case whose most probable state may go either way


def case_inputs(name):
    """(g, Q, child, blen, jc, n, tile) of a case of test_gpu_trees_loglik.CASES, built by that module's own helpers exactly as
    test_gpu_treegrad.py builds them"""
    from oracle import cpu_ref as O
    from test_gpu_trees_loglik import CASES, alignment, gtr_Q, random_trees, shaped_trees
    kw = CASES[name]
    N, S, jc, n = kw['N'], kw['S'], kw.get('jc', False), kw.get('n', T)
    g = alignment(N, S, 100 + N + S, kw.get('gaps', False), kw.get('generic', False))
    Q = O.jc_Q() if jc else gtr_Q()
    child, blen = shaped_trees(kw['shape'], N, 5, n) if 'shape' in kw else random_trees(N, 5, n)
    return g, Q, child, blen, jc, n, kw.get('tile')


def decided(post):
    """[...] bool: the two largest of post [...][4] differ by more than 2 TOL_ANC relative to the largest -- two computations
    within TOL_ANC of one another then agree on the most probable state (NaN columns: not decided)"""
    with np.errstate(invalid='ignore'):
        top = np.sort(post, axis=-1)
        return (top[..., 3] - top[..., 2]) > 2 * TOL_ANC * top[..., 3]


def within_tol(got, ref):
    """|got - ref| <= TOL_ANC |ref| where ref >= TINY, TOL_ANC TINY absolute below; returns (ok [...], worst error in units of the bound)"""
    bound = TOL_ANC * np.maximum(np.abs(ref), TINY)
    err = np.abs(got - ref) / bound
    return err <= 1.0, float(np.nanmax(err)) if err.size else 0.0


def gapped(N, S, rng):
    """indicator rows [N][S][4] of codes 0 .. 4, a 4 a gap (all ones)"""
    codes = rng.integers(0, 5, size=(N, S))
    return np.stack([(codes == b) | (codes == 4) for b in range(4)], axis=-1).astype(np.float64)
