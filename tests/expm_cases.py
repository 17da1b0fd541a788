"""The matrix function's contract: the grid of generators and lengths, the two references and the numbers
that tests/test_expm_contract_cpu.py and tests/test_gpu_expm_contract.py share.

  * the 50-digit reference: mpmath.expm(method='taylor') at 60 digits on the doubles fl(Q[i][j] * t) that pm_expm4 itself forms,
    taken exactly.  CPU only; its values are committed as tests/golden/expm_contract.npz (tests/golden/make_expm_contract.py), each
    as a double plus a double remainder.
  * the NumPy restatement of Higham 2005 Alg. 2.3 (`@`, np.linalg.solve, no fma, no attention to the order of operations): the
    yardstick of the tolerance, never the code under test.

The tolerance is fixed before any device runs:  TOL(name, s) = 2^s (8 E_REF0[name] + 4) u,  u = 2^-53, where E_REF0[name] is the
restatement's worst entrywise relative error (in u) over that generator's lengths without squarings; 8 is the project's margin
(DESIGN.md section 13); squaring a positive matrix whose entries carry relative error e gives 2 e + e^2, plus gamma_4 ~ 4 u from
the four-term fma chain: hence 2^s and + 4.
"""
import math
import os

import numpy as np

U = 2.0 ** -53
TINY = 2.0 ** -1000                      # entries whose true value lies below this are not compared relatively
THETA = (1.495585217958292e-2, 2.539398330063230e-1, 9.504178996162932e-1, 2.097847961257068e0, 5.371920351148152)
ORDER = (3, 5, 7, 9, 13)
PADE_B = {
    3: (120., 60., 12., 1.),
    5: (30240., 15120., 3360., 420., 30., 1.),
    7: (17297280., 8648640., 1995840., 277200., 25200., 1512., 56., 1.),
    9: (17643225600., 8821612800., 2075673600., 302702400., 30270240., 2162160., 110880., 3960., 90., 1.),
    13: (64764752532480000., 32382376266240000., 7771770303897600., 1187353796428800., 129060195264000., 10559470521600.,
         670442572800., 33522128640., 1323241920., 40840800., 960960., 16380., 182., 1.),
}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ('jc', 'hky50', 'skew', 'stiff', 'nonrev', 'softmax')

# The restatement's worst entrywise relative error over each generator's lengths without squarings, in u: measured by
# measure_e_ref0() against the 50-digit values (tests/golden/make_expm_contract.py prints them), rounded up to three digits.
E_REF0 = {'jc': 6.79, 'hky50': 11.4, 'skew': 105.0, 'stiff': 116.0, 'nonrev': 6.52, 'softmax': 7.68}

# The domain (phylo_treeset.h: PT2_EXPM_S_MAX, PT2_EXPM_NORM_MAX): the largest s with 2^s (8 max E_REF0 + 4) u <= 2^-20
S_MAX = max(s for s in range(64) if 2.0 ** s * (8 * max(E_REF0.values()) + 4) * U <= 2.0 ** -20)       # 23
NORM_MAX = THETA[4] * 2.0 ** S_MAX


def tol(name, s):
    return 2.0 ** s * (8 * E_REF0[name] + 4) * U


# ---- generators ---------------------------------------------------------------------------------------------------------------
def gtr(ex, pi):
    """unit mean rate, row-major: q_ij = r_ij pi_j off the diagonal; exchangeabilities (AC, AG, AT, CG, CT, GT)"""
    r = np.zeros((4, 4))
    r[0, 1], r[0, 2], r[0, 3], r[1, 2], r[1, 3], r[2, 3] = ex
    r = r + r.T
    pi = np.asarray(pi, dtype=np.float64)
    Q = r * pi[None, :]
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q / -(pi * np.diag(Q)).sum()


def generators():
    from phylo_amd import model
    y = 7.0 * np.random.default_rng(20).normal(size=(4, 4))           # a trained y_q far from its start: rates over e^+-14
    return {
        'jc': gtr((1, 1, 1, 1, 1, 1), (.25, .25, .25, .25)),
        'hky50': gtr((1, 50, 1, 1, 50, 1), (.1, .4, .2, .3)),
        'skew': gtr((1, 2, 1, 1, 2, 1), (.97, .01, .01, .01)),
        'stiff': gtr((1e-3, 1, 1e3, 1e3, 1, 1e-3), (.4, .1, .1, .4)),
        'nonrev': np.array(np.load(os.path.join(GOLDEN, "expm_tables.npz"))['Q/rand0'], dtype=np.float64),
        'softmax': model.get_Q(y),
    }


def norm1(Q):
    """||Q||_1 the way pm_expm4 adds it: the largest column sum of |q_ij|, rows in ascending order"""
    best = 0.0
    for j in range(4):
        cs = 0.0
        for i in range(4):
            cs = cs + abs(float(Q[i][j]))
        best = max(best, cs)
    return best


def kernel_norm_s(Q, t):
    """(||fl(Q t)||_1, s) as pm_expm4 computes them"""
    norm = norm1(np.asarray(Q, dtype=np.float64) * float(t))
    s, lim = 0, THETA[4]
    while norm > lim and s < 1000:
        lim, s = lim * 2.0, s + 1
    return norm, s


def lengths(Q):
    """the ~120 lengths of one generator"""
    n1 = norm1(Q)
    out = [0.0, -0.0, 5e-324, 1e-300, 1e-100, 1e-30, 1e-17, 1e-12, 1e-8, 1e-4]
    for th in THETA:                                      # class boundaries, and where s steps
        for k in (0, 1, 3, 6, 9, 12):
            b = th * 2.0 ** k / n1
            out += [np.nextafter(b, 0.0), np.nextafter(b, np.inf)]
    for s in (16, 20, 23):
        top = THETA[4] * 2.0 ** s / n1
        while n1 * top > THETA[4] * 2.0 ** s:              # the quotient rounded up: the largest length the host check lets through
            top = np.nextafter(top, 0.0)
        out += [0.5000001 * THETA[4] * 2.0 ** s / n1, 0.75 * THETA[4] * 2.0 ** s / n1, top]
    rng = np.random.default_rng(16)
    out += list(np.exp(rng.uniform(math.log(1e-6), math.log(THETA[4] / n1), 40)))
    return np.array(out, dtype=np.float64)


def in_domain(Q, t):
    """what pt2_check_expm_range accepts"""
    return norm1(Q) * np.abs(np.asarray(t, dtype=np.float64)) <= NORM_MAX


# ---- the 50-digit reference ---------------------------------------------------------------------------------------------------
def ref50(Q, t):
    """expm of the exact doubles fl(Q[i][j] t) at 60 digits -> (hi, lo) [4][4] doubles with hi + lo the value to ~106 bits"""
    import mpmath as mp
    A = np.asarray(Q, dtype=np.float64) * float(t)
    with mp.workdps(60):
        P = mp.expm(mp.matrix([[mp.mpf(float(v)) for v in row] for row in A]), method='taylor')
        hi = np.array([[float(P[i, j]) for j in range(4)] for i in range(4)])
        lo = np.array([[float(P[i, j] - mp.mpf(hi[i, j])) for j in range(4)] for i in range(4)])
    return hi, lo


def ref50_grid(Q, ts):
    hi, lo = np.empty((len(ts), 4, 4)), np.empty((len(ts), 4, 4))
    for k, t in enumerate(ts):
        hi[k], lo[k] = ref50(Q, t)
    return hi, lo


def jc_ref50(ts):
    """the JC69 matrix 1/4 + 3/4 e^-t | 1/4 - 1/4 e^-t at 60 digits -> (diag hi, diag lo, off hi, off lo)"""
    import mpmath as mp
    out = np.empty((4, len(ts)))
    with mp.workdps(60):
        for k, t in enumerate(ts):
            o = -mp.expm1(-mp.mpf(float(t))) / 4           # (1 - e^-t) / 4 without the cancellation at t = 1e-100
            d = 1 - 3 * o
            out[0, k] = float(d)
            out[1, k] = float(d - mp.mpf(out[0, k]))
            out[2, k] = float(o)
            out[3, k] = float(o - mp.mpf(out[2, k]))
    return out


def rel_err(P, hi, lo):
    """entrywise |P - (hi + lo)| / |hi| where |hi| >= TINY, else 0; in absolute terms, not in u"""
    P, hi, lo = np.asarray(P), np.asarray(hi), np.asarray(lo)
    with np.errstate(divide='ignore', invalid='ignore'):
        e = np.abs((P - hi) - lo) / np.abs(hi)
    return np.where(np.abs(hi) >= TINY, e, 0.0)


def contract():
    """everything tests/golden/expm_contract.npz holds, evaluated afresh (about ten seconds)"""
    out = {}
    for name, Q in generators().items():
        ts = lengths(Q)
        hi, lo = ref50_grid(Q, ts)
        out['Q/' + name], out['t/' + name], out['hi/' + name], out['lo/' + name] = Q, ts, hi, lo
    out['jc69/t'] = jc_lengths()
    out['jc69/ref'] = jc_ref50(out['jc69/t'])
    return out


def load_contract():
    return np.load(os.path.join(GOLDEN, "expm_contract.npz"))


# ---- the NumPy restatement ----------------------------------------------------------------------------------------------------
def restatement(Q, t):
    """Higham 2005 Alg. 2.3 in plain NumPy"""
    A = np.asarray(Q, dtype=np.float64) * float(t)
    norm = np.linalg.norm(A, 1)
    s = 0
    m = 13
    for th, order in zip(THETA, ORDER):
        if norm <= th:
            m = order
            break
    else:
        s = max(0, int(math.ceil(math.log2(norm / THETA[4]))))
        A = A / 2.0 ** s
    b = PADE_B[m]
    I = np.eye(4)
    A2 = A @ A
    if m < 13:
        pw = [I, A2]
        for _ in range(2, (m + 1) // 2):
            pw.append(pw[-1] @ A2)
        Uo = A @ sum(b[2 * k + 1] * pw[k] for k in range(len(pw)))
        V = sum(b[2 * k] * pw[k] for k in range(len(pw)))
    else:
        A4 = A2 @ A2
        A6 = A4 @ A2
        Uo = A @ (A6 @ (b[13] * A6 + b[11] * A4 + b[9] * A2) + b[7] * A6 + b[5] * A4 + b[3] * A2 + b[1] * I)
        V = A6 @ (b[12] * A6 + b[10] * A4 + b[8] * A2) + b[6] * A6 + b[4] * A4 + b[2] * A2 + b[0] * I
    P = np.linalg.solve(V - Uo, V + Uo)
    for _ in range(s):
        P = P @ P
    return P


def measure_e_ref0(name, Q, ts, hi, lo):
    """the restatement's worst entrywise relative error, in u, over the lengths without squarings"""
    worst = 0.0
    for k, t in enumerate(ts):
        if kernel_norm_s(Q, t)[1] == 0:
            worst = max(worst, float(rel_err(restatement(Q, t), hi[k], lo[k]).max()) / U)
    return worst


# ---- the JC closed form's lengths ---------------------------------------------------------------------------------------------
def jc_lengths():
    fixed = [0.0, -0.0, 5e-324, 1e-300, 1e-100, 1e-30, 1e-17, 1e-12, 1e-8, 1e-4, 2.0 ** -54, np.nextafter(2.0 ** -54, 0.0), 2.0 ** -53,
             2.0 ** -28, np.nextafter(2.0 ** -28, 0.0), 0.34657359027997264, 1.0, 700.0, 745.2, 1e100, 1e300]
    rng = np.random.default_rng(69)
    return np.concatenate([fixed, np.exp(rng.uniform(-40.0, 6.0, 2000))])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_jc_closed_form(P, ts, ref, what):
    """absolute error off-diagonal <= 0.5 u, diagonal <= 2 u; off-diagonal relative error <= 4 u /
    min(t, 1); off-diagonal exactly 0 below 2^-54; rows within 4 u of 1"""
    d, o = P[:, 0, 0], P[:, 0, 1]
    eye = np.eye(4, dtype=bool)
    assert np.array_equal(bits(P[:, eye]), bits(np.repeat(d[:, None], 4, 1))), what
    assert np.array_equal(bits(P[:, ~eye]), bits(np.repeat(o[:, None], 12, 1))), what
    dh, dl, oh, ol = ref
    ea_d, ea_o = np.abs((d - dh) - dl), np.abs((o - oh) - ol)
    assert ea_o.max() <= 0.5 * U and ea_d.max() <= 2 * U, (what, ea_o.max() / U, ea_d.max() / U)
    pos = oh >= TINY                                                       # (all but t = +-0 and 5e-324)
    assert np.sum(~pos) == 3
    er = ea_o[pos] / oh[pos] * np.minimum(ts[pos], 1.0)
    assert er.max() <= 4 * U, (what, er.max() / U)
    assert np.all(o[np.abs(ts) < 2.0 ** -54] == 0.0) and np.all(o >= 0.0) and np.all(d <= 1.0), what
    rows = np.abs(np.array([math.fsum((a, b, b, b)) for a, b in zip(d, o)]) - 1.0)
    assert rows.max() <= 4 * U, (what, rows.max() / U)
    big = ts >= 1e100
    assert big.sum() == 2 and np.all(P[big] == 0.25)
    return ea_o.max() / U, ea_d.max() / U, er.max() / U
