"""The matrix function's contract on the device (tests/expm_cases.py).

  * the grid: pk_expm_batched is bit-equal to the C oracle and -- independently of the oracle -- within TOL(name, s) of the 50-digit
    values of tests/golden/expm_contract.npz;
  * divergent waves: one matrix per lane, so neighbouring lanes take different Pade branches and squaring counts; a length's 16
    outputs carry the same bits wherever it sits, in any order and with a ragged last wave;
  * the JC69 closed form: bit-equal to the oracle, exact in absolute terms;
  * what the tree-set calls use: a two-leaf tree with lengths (t, 0) returns prior_b P(t)[a][b] per site, the matrix being
    expm_batched's, and under one rate category the matrix of the single rounded product fl(r t);
  * refusals: a length whose matrix has lost its digits is PHYLO_EINVAL naming tree and row, nothing is queued, and the JC69
    closed form has no limit."""
import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import cpu_ref as O
from phylo_amd import _ffi
from tests import expm_cases as X

pytestmark = pytest.mark.gpu
U = X.U
bits = X.bits
PRIOR = np.array([0.1, 0.2, 0.3, 0.4])


def pair_leaves():
    """N = 2 coded leaves, S = 16 sites: site 4 a + b shows state a at leaf 0 and state b at leaf 1"""
    g = np.zeros((2, 16, 4))
    for a in range(4):
        for b in range(4):
            g[0, 4 * a + b, a] = 1.0
            g[1, 4 * a + b, b] = 1.0
    return g


def make_ctx(Q, jc=False, g=None):
    g = pair_leaves() if g is None else g
    N, S, _ = g.shape
    ctx = _ffi.Context(2, N, S)
    ctx.set_leaves(g)
    ctx.set_model(Q, np.full((1, 4), 0.25), np.full(N - 1, 10.0), np.full(N - 1, 10.0), jc69_closed_form=jc)
    return ctx


@pytest.fixture(scope="module")
def npz():
    return X.load_contract()


# ---- the grid ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.NAMES)
def test_grid_bit_equal_to_oracle_and_within_tol_of_50_digits(npz, name):
    Q, ts, hi, lo = npz['Q/' + name], npz['t/' + name], npz['hi/' + name], npz['lo/' + name]
    with make_ctx(Q) as ctx:
        P = ctx.expm_batched(ts)
    assert np.array_equal(bits(P), bits(CO.expm_batched(Q, ts))), name
    assert np.all(np.isfinite(P)) and np.all(P >= 0.0), name
    worst = 0.0
    for k, t in enumerate(ts):
        T = X.tol(name, X.kernel_norm_s(Q, t)[1])
        e = float(X.rel_err(P[k], hi[k], lo[k]).max())
        worst = max(worst, e / T)
        assert e <= T, "%s t=%r: relative error %.3g u over TOL %.3g u" % (name, t, e / U, T / U)
        if t == 0.0:
            assert np.array_equal(bits(P[k]), bits(np.eye(4))), (name, t)
    print("%s: worst error / TOL %.4f; %.1f %% of the entries are the correctly rounded 50-digit value"
          % (name, worst, 100.0 * np.mean(bits(P) == bits(hi))))


# ---- divergent waves --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.NAMES)
def test_a_length_has_the_same_bits_wherever_it_sits(npz, name):
    Q = npz['Q/' + name]
    grid = np.concatenate([npz['t/' + n] for n in X.NAMES])
    grid = grid[X.in_domain(Q, grid)]                       # the lengths of every generator this one takes: ~700, s from 0 to 23
    assert len(grid) > 650
    rng = np.random.default_rng(5)
    with make_ctx(Q) as ctx:
        order = np.argsort(grid, kind='stable')
        ref = np.empty((len(grid), 4, 4))
        ref[order] = ctx.expm_batched(grid[order])          # sorted: neighbours agree as far as they can
        assert np.array_equal(bits(ref), bits(CO.expm_batched(Q, grid))), name
        for what, perm in (("reversed", order[::-1]), ("shuffled", rng.permutation(len(grid)))):
            assert np.array_equal(bits(ctx.expm_batched(grid[perm])), bits(ref[perm])), (name, what)
        pick = rng.integers(0, len(grid), 4097)
        for n in (1, 63, 64, 65, 4097):                     # a ragged last wave
            P = ctx.expm_batched(grid[pick[:n]])
            assert P.shape == (n, 4, 4) and np.array_equal(bits(P), bits(ref[pick[:n]])), (name, n)


# ---- the JC69 closed form ---------------------------------------------------------------------------------------------------
def test_jc_closed_form_on_the_device(npz):
    ts, ref = npz['jc69/t'], npz['jc69/ref']
    with make_ctx(O.jc_Q(), jc=True) as ctx:
        P = ctx.expm_batched(ts)
    assert np.array_equal(bits(P), bits(CO.expm_batched(O.jc_Q(), ts, jc=True)))
    eo, ed, er = X.check_jc_closed_form(P, ts, ref, "device")
    print("JC69 closed form: off-diagonal %.3f u, diagonal %.3f u absolute; off-diagonal %.3f u / min(t, 1) relative" % (eo, ed, er))


# ---- what the tree-set calls use --------------------------------------------------------------------------------------------
def pair_lengths(Q):
    """three class boundaries (theta_3 from above, theta_7 from below, theta_13 from above), one length with six squarings, 1e-8"""
    n1 = X.norm1(Q)
    ts = [np.nextafter(X.THETA[0] / n1, np.inf), np.nextafter(X.THETA[2] / n1, 0.0), np.nextafter(X.THETA[4] / n1, np.inf),
          0.75 * X.THETA[4] * 64.0 / n1, 1e-8]
    assert X.kernel_norm_s(Q, ts[3])[1] == 6
    return np.array(ts)


def expected_sites(P, side):
    """a two-leaf tree with lengths (t, 0): the zero-length side is the identity, so site (a, b) is prior_b P[a][b] (a partial is
    the child's row times the matrix: DESIGN.md section 11); with (0, t) it is prior_a P[b][a]"""
    out = np.empty(16)
    for a in range(4):
        for b in range(4):
            out[4 * a + b] = PRIOR[b] * P[a, b] if side == 0 else PRIOR[a] * P[b, a]
    return out


def check_pair_trees(ctx, ts, call, matrices, what):
    child = np.tile(np.array([[[0, 1]]], dtype=np.int32), (2 * len(ts), 1, 1))
    blen = np.zeros((2 * len(ts), 1, 2))
    blen[:len(ts), 0, 0] = ts                               # (t, 0)
    blen[len(ts):, 0, 1] = ts                               # (0, t)
    ll, sites = call(child, blen)
    same = 0
    for k in range(2 * len(ts)):
        want = expected_sites(matrices[k % len(ts)], k // len(ts))
        assert np.all(want > 0.0)
        err = np.abs(sites[k] - want) / want
        assert err.max() <= 2 * U, (what, k, err.max() / U)
        same += int(np.array_equal(bits(sites[k]), bits(want)))
        assert abs(ll[k] - np.log(want).sum()) <= 1e-13 * abs(ll[k])
    print("%s: %d of %d trees carry the product's bits at every site" % (what, same, 2 * len(ts)))


@pytest.mark.parametrize("jc", [False, True])
def test_tree_set_calls_use_the_matrices_of_expm_batched(jc):
    Q = O.jc_Q() if jc else X.generators()['nonrev']
    ts = pair_lengths(Q)
    with make_ctx(Q, jc=jc) as ctx:
        P = ctx.expm_batched(ts)
        if not jc:
            assert np.abs(P[3] - P[3].T).max() > 1e-3       # a transposed matrix would show
        check_pair_trees(ctx, ts, lambda c, b: ctx.trees_loglik(c, b, prior=PRIOR, want_sites=True), P, "trees_loglik, jc=%r" % jc)
        for r in (1e-12, 0.37, 7.5) if not jc else (0.37,):
            Pr = ctx.expm_batched(r * ts)                   # the matrix of the single rounded product fl(r t)
            check_pair_trees(ctx, ts, lambda c, b: ctx.trees_loglik_rates(c, b, [r], [1.0], prior=PRIOR, want_sites=True), Pr,
                             "trees_loglik_rates, rate %g, jc=%r" % (r, jc))


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def four_leaves():
    rng = np.random.default_rng(3)
    g = np.zeros((4, 40, 4))
    codes = rng.integers(0, 4, (4, 40))
    for n in range(4):
        g[n, np.arange(40), codes[n]] = 1.0
    return g


def test_lengths_outside_the_domain_are_refused():
    Q = X.generators()['nonrev']
    n1 = X.norm1(Q)
    top = X.NORM_MAX / n1
    while n1 * top > X.NORM_MAX:
        top = np.nextafter(top, 0.0)
    while n1 * np.nextafter(top, np.inf) <= X.NORM_MAX:
        top = np.nextafter(top, np.inf)
    over = np.nextafter(top, np.inf)
    child = np.tile(np.array([[0, 1], [4, 2], [5, 3]], dtype=np.int32), (3, 1, 1))
    blen = np.random.default_rng(4).uniform(0.01, 0.5, (3, 3, 2))
    rates, weights = np.array([0.2, 7.5]), np.array([0.5, 0.5])
    dirs = np.zeros((1, 4, 4)); dirs[0, 0, 1], dirs[0, 0, 0] = 1.0, -1.0
    g = four_leaves()
    with make_ctx(Q, g=g) as ctx:
        calls = {
            'trees_loglik': lambda b: ctx.trees_loglik(child, b, prior=PRIOR, want_sites=True),
            'trees_grad': lambda b: ctx.trees_grad(child, b, prior=PRIOR),
            'trees_ancestral': lambda b: ctx.trees_ancestral(child, b, prior=PRIOR),
            'trees_grad_model': lambda b: ctx.trees_grad_model(child, b, dirs, prior=PRIOR),
            'trees_nni': lambda b: ctx.trees_nni(child, b, prior=PRIOR),
        }
        rate_calls = {
            'trees_loglik_rates': lambda b: ctx.trees_loglik_rates(child, b, rates, weights, prior=PRIOR, want_sites=True),
            'trees_grad_rates': lambda b: ctx.trees_grad_rates(child, b, rates, weights, prior=PRIOR),
            'trees_ancestral_rates': lambda b: ctx.trees_ancestral_rates(child, b, rates, weights, prior=PRIOR),
            'trees_nni_rates': lambda b: ctx.trees_nni_rates(child, b, rates, weights, prior=PRIOR),
        }
        before = {k: f(blen) for k, f in {**calls, **rate_calls}.items()}
        P_before = ctx.expm_batched([0.1, top])

        def same(a, b, what):
            a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
            for x, y in zip(a, b):
                x, y = np.asarray(x), np.asarray(y)
                if x.dtype == np.float64:
                    assert np.array_equal(bits(x), bits(y)), what
                else:
                    assert np.array_equal(x, y), what

        def refused(call, *words):
            with pytest.raises(_ffi.PhyloError) as e:
                call()
            assert e.value.code == -1, str(e.value)
            for w in words:
                assert w in str(e.value), (w, str(e.value))

        # the matrix function itself: the largest length it takes, and its neighbour
        refused(lambda: ctx.expm_batched([0.1, 0.2, over]), 't[2]', 'above 4.50629e+07')
        refused(lambda: ctx.expm_batched([1e100]), 't[0]', 'length 1e+100', 'above 4.50629e+07')
        refused(lambda: ctx.expm_batched([0.1, -over]), 't[1]')
        refused(lambda: ctx.expm_batched([np.inf]), 't[0]')
        same(ctx.expm_batched([0.1, top]), P_before, "expm_batched after a refusal")
        # every tree-set call: tree 2, row 1 carries the length
        for bad in (over, 1e100):
            b = blen.copy(); b[2, 1, 1] = bad
            for k, f in calls.items():
                refused(lambda: f(b), 'tree 2, row 1:', 'length %g' % bad, 'above 4.50629e+07')
                same(f(blen), before[k], k + " after a refusal")
        b = blen.copy(); b[2, 1, 1] = top                    # the limit itself is inside
        assert np.all(np.isfinite(ctx.trees_loglik(child, b, prior=PRIOR)))
        # the rates calls: rate * length is what counts
        b = blen.copy(); b[1, 2, 0] = top / 7.0             # fine at rate 0.2, over at rate 7.5
        assert np.all(np.isfinite(calls['trees_loglik'](b)[0]))
        for k, f in rate_calls.items():
            refused(lambda: f(b), 'tree 1, row 2, category 1:', 'at rate 7.5', 'above 4.50629e+07')
            same(f(blen), before[k], k + " after a refusal")
        # the single-tree call
        left, right = np.array([0, 0, 0, 0, 0, 4, 5], dtype=np.int32), np.array([0, 0, 0, 0, 1, 2, 3], dtype=np.int32)
        bl, br = np.array([0, 0, 0, 0, 0.1, 0.2, 0.3]), np.array([0, 0, 0, 0, 0.1, 1e100, 0.3])
        ok, _ = ctx.tree_loglik(left, right, bl, np.array([0, 0, 0, 0, 0.1, 0.2, 0.3]), 6, g, PRIOR)
        refused(lambda: ctx.tree_loglik(left, right, bl, br, 6, g, PRIOR), 'tree 0, row 5:', 'length 1e+100')
        assert ctx.tree_loglik(left, right, bl, np.array([0, 0, 0, 0, 0.1, 0.2, 0.3]), 6, g, PRIOR)[0] == ok
    # under the JC69 closed form there is no limit: 1/4 everywhere
    with make_ctx(O.jc_Q(), jc=True, g=g) as ctx:
        assert np.all(ctx.expm_batched([1e100, 1e300, np.inf]) == 0.25)
        b = blen.copy(); b[2, 1, 1] = 1e100
        ll, sites = ctx.trees_loglik(child, b, prior=PRIOR, want_sites=True)
        assert np.all(np.isfinite(ll)) and np.all(sites > 0.0)
        ll_r = ctx.trees_loglik_rates(child, b, rates, weights, prior=PRIOR)
        assert np.all(np.isfinite(ll_r))
    with make_ctx(O.jc_Q(), jc=True) as ctx:                 # the pair tree at 1e100: every site is prior_b / 4
        _, sites = ctx.trees_loglik(np.array([[[0, 1]]], dtype=np.int32), np.array([[[1e100, 0.0]]]), prior=PRIOR, want_sites=True)
        assert np.array_equal(sites[0], np.tile(PRIOR * 0.25, 4))
