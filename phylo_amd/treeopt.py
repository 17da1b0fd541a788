"""Maximum-likelihood branch lengths of a set of trees: a driver in plain NumPy over a function that returns
the log-likelihood of every tree with its gradient and own second derivatives (Context.trees_grad on the device, any restatement
of it in the tests).  No device code here."""
import numpy as np

EPS_CURV = 1e-6          # a curvature above -EPS_CURV (flat or convex along the branch) is taken for -EPS_CURV
ARMIJO = 1e-4            # a step is accepted when the log-likelihood rises by at least this share of what the gradient promises
NOISE = 2.0 ** -46       # two log-likelihoods closer than this share of their size are told apart by their gradients (see below)
MEMORY = 8               # pairs (change of lengths, change of gradient) a tree keeps for its quasi-Newton correction
MIN_FACTOR = 2.0 ** -4   # a tree whose step factor falls below this forgets its pairs: the plain diagonal step is an ascent direction


class OutOfRangeError(ValueError):
    """a tree cannot be climbed from its starting lengths: its log-likelihood or its derivatives are not finite there"""


def _free(b, g, lo, hi):
    """branches that may move: not at a bound with the gradient pointing outward"""
    return ~(((b <= lo) & (g < 0)) | ((b >= hi) & (g > 0)))


def _converged(b, g, lo, hi, gtol):
    """per tree: every branch has |g| <= gtol, or sits at a bound with the gradient pointing outward"""
    ok = (np.abs(g) <= gtol) | ~_free(b, g, lo, hi)
    return ok.all(axis=1)


def _direction(g, c, free, mem, b):
    """Per tree the ascent direction: the diagonal Newton step -g / min(c, -EPS_CURV) of every free branch, corrected by the
    tree's remembered pairs (the two-loop recursion of L-BFGS with the diagonal Newton matrix as its initial matrix; with no
    pair remembered it IS the diagonal step).  g, c, free, b [T][n]; mem a list of (s, y, rho) with rho [T] (0 = pair not held)."""
    h0 = -1.0 / np.minimum(c, -EPS_CURV)
    q = np.where(free, g, 0.0)
    alphas = []
    for s, y, rho in reversed(mem):
        a = rho * (s * q).sum(axis=1)
        q = q - a[:, None] * y
        alphas.append(a)
    d = h0 * q
    for (s, y, rho), a in zip(mem, reversed(alphas)):
        beta = rho * (y * d).sum(axis=1)
        d = d + (a - beta)[:, None] * s
    d = np.where(free, d, 0.0)
    plain = np.where(free, h0 * g, 0.0)
    bad = ~np.isfinite(d).all(axis=1) | ((g * d).sum(axis=1) <= 0)
    d[bad] = plain[bad]
    cap = np.maximum(1.0, b)                                # no branch moves by more than its own length (or 1) in one step: a flat or
    return np.clip(d, -cap, cap), bad                       # convex branch (curvature taken for -EPS_CURV) would otherwise jump to a bound


def optimize_branches(grad_fn, child, blen, lo=1e-8, hi=100.0, max_iter=50, gtol=1e-6):
    """Climb the log-likelihood of T trees over their branch lengths.  grad_fn(blen [T][N-1][2]) -> (loglik [T], grad, curv) for
    all trees at once; child is carried for the caller (grad_fn knows the topologies).  lo and hi are numbers, or arrays of
    blen's shape without its first axis (a bound per coordinate).

    All trees advance in lockstep, one call of grad_fn per iteration.  A tree's trial point is its current lengths plus its
    step factor times its direction, projected onto [lo, hi].  The direction is the diagonal Newton step -g / min(curv,
    -EPS_CURV) of every branch; because branches that share a degree of freedom (the two at the root under a reversible model,
    the branches round an internal branch of length zero) make that step alone swing about the optimum or crawl, a tree also
    remembers its last MEMORY accepted steps and corrects the direction by them (L-BFGS over the diagonal Newton matrix).  The
    trial is accepted when the tree's log-likelihood does not fall and rises by ARMIJO of the first-order promise (a promise
    below the rounding of the log-likelihood is not asked for); otherwise the tree keeps its lengths and its factor is halved.
    A trial whose log-likelihood, gradient or curvature is not finite is refused like one that falls: phylo_trees_grad gives NaN
    derivatives beside a finite log-likelihood to a tree with a site factor below 2^-1020, and there is
    nothing to climb on there.  A tree in that state at the STARTING lengths raises OutOfRangeError (a ValueError) naming it.
    After an accepted step the factor is 1 again.  A tree's lengths change on accepted steps only: its sequence of
    log-likelihoods never falls.  A tree is converged when every branch has |g| <= gtol or sits at a bound with the gradient
    pointing outward.

    Returns a dict: 'blen' [T][N-1][2], 'loglik' [T], 'iterations' [T] (calls of grad_fn while the tree was not converged),
    'converged' [T] bool, 'grad' [T][N-1][2] at the returned lengths, 'history' [calls + 1][T] the log-likelihood of every tree
    at the start and after every call."""
    del child
    b = np.array(blen, dtype=np.float64)
    if b.ndim == 2:
        b = b[None]
    shape = b.shape
    T = shape[0]
    b = b.reshape(T, -1)
    if np.ndim(lo):                                         # bounds per coordinate (optimize_rates): one row for all trees
        lo = np.asarray(lo, dtype=np.float64).reshape(-1)
    if np.ndim(hi):
        hi = np.asarray(hi, dtype=np.float64).reshape(-1)
    b = np.clip(b, lo, hi)

    def call(x):
        ll, g, c = grad_fn(x.reshape(shape))
        return np.array(ll, dtype=np.float64), np.array(g, dtype=np.float64).reshape(T, -1), np.array(c, dtype=np.float64).reshape(T, -1)

    ll, g, c = call(b)
    for t in range(T):
        if not np.isfinite(ll[t]):
            raise OutOfRangeError("optimize_branches: the log-likelihood of tree %d is not finite at the starting lengths" % t)
        if not (np.isfinite(g[t]).all() and np.isfinite(c[t]).all()):
            raise OutOfRangeError("optimize_branches: the gradient of tree %d is not finite at the starting lengths (log-likelihood "
                                  "%.17g): a site likelihood lies below 2^-1020, outside the range of phylo_trees_grad" % (t, ll[t]))
    factor = np.ones(T)
    iters = np.zeros(T, dtype=np.int64)
    history = [ll.copy()]
    mem = []
    free_was = _free(b, g, lo, hi)
    done = _converged(b, g, lo, hi, gtol)
    for _ in range(max_iter):
        if done.all():
            break
        free = _free(b, g, lo, hi)
        d, bad = _direction(g, c, free, mem, b)
        forget = bad | (factor < MIN_FACTOR) | (free != free_was).any(axis=1)      # (pairs made with another set of moving branches mislead)
        free_was = free
        if forget.any():
            for _, _, rho in mem:
                rho[forget] = 0.0
            plain, _ = _direction(g, c, free, [], b)
            d[forget] = plain[forget]
        trial = np.clip(b + factor[:, None] * d, lo, hi)
        trial[done] = b[done]
        promise = (g * (trial - b)).sum(axis=1)
        ll_t, g_t, c_t = call(trial)
        iters[~done] += 1
        with np.errstate(invalid='ignore'):
            # Inside the rounding of the sum over sites the difference of two log-likelihoods says nothing, while the gradients at
            # both ends still do: there the rise is judged by the trapezoid (g + g_t) . step / 2, and the tree's log-likelihood
            # keeps the larger of the two computed values (they differ by less than NOISE |loglik|).
            near = np.abs(ll_t - ll) <= NOISE * np.abs(ll)
            rise = 0.5 * ((g + g_t) * (trial - b)).sum(axis=1)
            ok_t = np.isfinite(ll_t) & np.isfinite(g_t).all(axis=1) & np.isfinite(c_t).all(axis=1)
            take = ~done & ok_t & np.where(near, rise >= 0, (ll_t >= ll) & (ll_t - ll >= ARMIJO * promise))
        ll_t = np.where(near & ok_t, np.maximum(ll, ll_t), ll_t)
        s, y = trial - b, g - g_t                           # (y of -loglik: positive curvature).  Accepted steps only: a refused trial
        sy = (s * y).sum(axis=1)                            # may lie where the surface is nothing like it is here
        keep = take & (sy > 1e-300)
        s, y = np.where(keep[:, None], s, 0.0), np.where(keep[:, None], y, 0.0)
        rho = np.where(keep, 1.0 / np.where(keep, sy, 1.0), 0.0)
        mem = (mem + [(s, y, rho)])[-MEMORY:]
        b[take], ll[take], g[take], c[take] = trial[take], ll_t[take], g_t[take], c_t[take]
        factor[take] = 1.0
        factor[~take & ~done] *= 0.5
        history.append(ll.copy())
        done = _converged(b, g, lo, hi, gtol)
    return {'blen': b.reshape(shape), 'loglik': ll, 'iterations': iters, 'converged': done, 'grad': g.reshape(shape),
            'history': np.array(history)}


ALPHA_BOUNDS = (0.02, 100.0)     # the shape of the discrete Gamma model, fitted as log alpha
PINV_BOUNDS = (0.0, 0.99)        # the share of invariant sites, fitted as it is: 0 is a value it may take (logit cannot)
FIRST_STEP = 0.1                 # the first step of a model coordinate is at most this (they have no device curvature)


def optimize_rates(grad_fn, child, blen, alpha0, C, pinv0=None, fit=('alpha',), lo=1e-8, hi=100.0, max_iter=200, gtol=1e-6):
    """Climb the mixture log-likelihood of T trees over their branch lengths AND, per tree, the shape alpha of a discrete Gamma
    model of C categories ('alpha' in fit) and the share p_inv of invariant sites ('pinv' in fit); fit=() climbs the lengths
    alone under the given model.  grad_fn(blen [T][N-1][2], rates [T][C'], weights [T][C']) -> (loglik [T], grad, curv,
    drate [T][C'], dweight [T][C']): Context.trees_grad_rates on the device (a mixture per tree), or a restatement of it.

    Every tree climbs in lockstep through optimize_branches, one call of grad_fn per iteration.  A tree's coordinates are its
    2 (N-1) lengths, then log alpha (bounds ALPHA_BOUNDS on alpha), then p_inv itself (bounds PINV_BOUNDS).  The mixture of a
    tree is phylo_amd.rates.rate_model(alpha, C, p_inv) with the invariant class kept whenever p_inv is fitted or starts above
    0 (a class of weight 0 is an ordinary category), the model coordinates' gradient phylo_amd.rates.chain of drate and dweight
    with rate_model_jacobian.  They have no curvature from the device: a tree's takes the fixed value -max(|g0|, 1) /
    FIRST_STEP, g0 its gradient at the start, so that a first step is of order FIRST_STEP; the remembered pairs of
    optimize_branches then supply what couples them to the lengths.  alpha0 and pinv0 are numbers or [T].
    max_iter is 200: under a Gamma model with many slow sites a wrong topology's internal branches run into their lower bound one
    after the other, and every change of the set of moving branches drops the remembered pairs (measured: 8 taxa, 260 sites,
    alpha 0.33 -- 32 to 129 iterations for the lengths alone, 39 to 139 with alpha).

    Returns what optimize_branches returns ('grad' the lengths' [T][N-1][2]), and per tree 'alpha', 'pinv' [T] (None where the
    model has no such class), 'rates', 'weights' [T][C'] and 'grad_model' [T][k], the gradient of the fitted model coordinates."""
    from . import rates as rates_mod
    fit = tuple(fit)
    if any(f not in ('alpha', 'pinv') for f in fit):
        raise ValueError("optimize_rates: fit holds 'alpha' and 'pinv', not %r" % (fit,))
    b0 = np.array(blen, dtype=np.float64)
    if b0.ndim == 2:
        b0 = b0[None]
    T, nb = b0.shape[0], b0[0].size
    alpha_start = np.broadcast_to(np.asarray(alpha0, dtype=np.float64), (T,)).copy()
    has_inv = 'pinv' in fit or (pinv0 is not None and np.any(np.asarray(pinv0, dtype=np.float64) > 0))
    pinv_start = np.broadcast_to(np.asarray(0.0 if pinv0 is None else pinv0, dtype=np.float64), (T,)).copy()
    fit_a, fit_p = 'alpha' in fit, 'pinv' in fit
    k = int(fit_a) + int(fit_p)
    x0 = np.concatenate([b0.reshape(T, nb)] + ([np.log(alpha_start)[:, None]] if fit_a else []) + ([pinv_start[:, None]] if fit_p else []),
                        axis=1)
    los = np.concatenate([np.full(nb, lo)] + ([[np.log(ALPHA_BOUNDS[0])]] if fit_a else []) + ([[PINV_BOUNDS[0]]] if fit_p else []))
    his = np.concatenate([np.full(nb, hi)] + ([[np.log(ALPHA_BOUNDS[1])]] if fit_a else []) + ([[PINV_BOUNDS[1]]] if fit_p else []))
    models = {}                                             # (alpha, p_inv) -> rates, weights and their Jacobian: a converged tree asks again

    def model_of(a, p):
        key = (float(a), float(p))
        if key not in models:
            models[key] = rates_mod.rate_model(key[0], C, key[1], keep_invariant=has_inv) + \
                rates_mod.rate_model_jacobian(key[0], C, key[1], keep_invariant=has_inv)
        return models[key]

    curv_model = [None]

    def unpack(x):
        a = np.exp(x[:, nb]) if fit_a else alpha_start
        p = x[:, nb + int(fit_a)] if fit_p else pinv_start
        ms = [model_of(a[t], p[t]) for t in range(T)]
        return a, p, ms, np.array([m[0] for m in ms]), np.array([m[1] for m in ms])

    def fn(x):
        x = x.reshape(T, nb + k)
        a, p, ms, rt, wt = unpack(x)
        ll, g, c, drate, dweight = grad_fn(x[:, :nb].reshape(b0.shape), rt, wt)
        da, dp = rates_mod.chain(drate, dweight, (np.array([m[2] for m in ms]), np.array([m[3] for m in ms])))
        gm = np.stack(([da * a] if fit_a else []) + ([dp] if fit_p else []), axis=1) if k else np.empty((T, 0))
        if curv_model[0] is None:                           # the first call: the starting point
            with np.errstate(invalid='ignore'):
                curv_model[0] = -np.maximum(np.abs(np.nan_to_num(gm)), 1.0) / FIRST_STEP
        g = np.concatenate([np.asarray(g, dtype=np.float64).reshape(T, nb), gm], axis=1)
        c = np.concatenate([np.asarray(c, dtype=np.float64).reshape(T, nb), curv_model[0]], axis=1)
        return ll, g[:, :, None], c[:, :, None]

    out = optimize_branches(fn, child, x0[:, :, None], lo=los[:, None], hi=his[:, None], max_iter=max_iter, gtol=gtol)
    x = out['blen'].reshape(T, nb + k)
    a, p, _, rt, wt = unpack(x)                             # the models of the returned point (cached: no new quantiles)
    g = out['grad'].reshape(T, nb + k)
    out.update(blen=x[:, :nb].reshape(b0.shape), grad=g[:, :nb].reshape(b0.shape), grad_model=g[:, nb:],
               alpha=np.array(a), pinv=np.array(p) if has_inv else None, rates=rt, weights=wt)
    return out


MODEL_ITER = 200                 # quasi-Newton steps of one model fit at fixed lengths
MODEL_HALVINGS = 40              # step halvings of one line search before the fit gives up


def _climb_bfgs(fun, x0, gtol, max_iter=MODEL_ITER):
    """Maximise fun(x) -> (f, g) from x0 by BFGS with backtracking: the inverse matrix starts as the identity scaled so that the
    first step is of order FIRST_STEP and takes the usual scaling s.y / y.y after the first accepted step.  A trial is taken when
    f does not fall and rises by ARMIJO of the first-order promise; two values closer than NOISE of their size are told apart
    by the trapezoid of their gradients (optimize_branches' rule).  Returns the point of the largest f seen, its f and g, the
    steps taken and the list of f."""
    x = np.array(x0, dtype=np.float64)
    f, g = fun(x)
    if not (np.isfinite(f) and np.isfinite(g).all()):
        raise OutOfRangeError("optimize_model: the objective or its gradient is not finite at the starting model")
    n = x.size
    H = np.eye(n) * (FIRST_STEP / max(np.abs(g).max(), 1.0))
    fs, steps, first = [f], 0, True
    best = (x, f, g)                                        # inside NOISE a step judged by its gradients may lower f: the best point is returned
    for _ in range(max_iter):
        if np.abs(g).max() <= gtol:
            break
        d = H @ g
        if not np.isfinite(d).all() or g @ d <= 0:
            H = np.eye(n) * (FIRST_STEP / max(np.abs(g).max(), 1.0))
            d = H @ g
        step, taken = 1.0, False
        for _ in range(MODEL_HALVINGS):
            xt = x + step * d
            ft, gt = fun(xt)
            if np.isfinite(ft) and np.isfinite(gt).all():
                if abs(ft - f) <= NOISE * abs(f):
                    ok = 0.5 * ((g + gt) @ (xt - x)) >= 0
                else:
                    ok = ft >= f and ft - f >= ARMIJO * step * (g @ d)
                if ok:
                    taken = True
                    break
            step *= 0.5
        if not taken:
            break
        s, y = xt - x, g - gt
        sy = s @ y
        if sy > 1e-300:
            if first:
                H = np.eye(n) * (sy / (y @ y))
                first = False
            rho = 1.0 / sy
            V = np.eye(n) - rho * np.outer(s, y)
            H = V @ H @ V.T + rho * np.outer(s, s)
        moved = np.abs(s).max()
        x, f, g = xt, ft, gt
        if f >= best[1]:
            best = (x, f, g)
        fs.append(f)
        steps += 1
        if moved == 0.0:
            break
    return best[0], best[1], best[2], steps, fs


def optimize_model(grad_model_fn, grad_fn, child, blen, y_q0, y_station0, fit=('q',), fit_on=None, max_rounds=20, tol=1e-6,
                   lo=1e-8, hi=100.0, branch_iter=50, gtol=1e-6):
    """Fit ONE substitution model shared by T trees, and every tree's branch lengths under it, by climbing the log-likelihood
    grad_fn and grad_model_fn compute.  CAVEAT: on the device that function is the project's, whose pruning step is x . M (SURVEY.md
    quirk Q2); for an asymmetric Q its site factors are not probabilities, it has no interior maximum over Q, and the climb ends on
    the boundary of the softmax -- the result is then NOT a maximum-likelihood estimate of a substitution model (DESIGN.md section
    13c).  Over functions whose factors are probabilities (the textbook convention) it is one.  The model: the
    project's row-softmax Q (phylo_amd.model.get_Q of y_q; 'q' in fit, always) and the root distribution softmax(y_station)
    ('pi' in fit).  Block-coordinate ascent:

      (a) every tree's lengths are climbed by optimize_branches under the current model;
      (b) with the lengths fixed, BFGS with backtracking climbs the twelve off-diagonal entries of y_q (and the four of
          y_station, whose gradient has no component along (1, 1, 1, 1): fifteen free coordinates at most) on the objective
          sum over t in fit_on of loglik[t].

    fit_on defaults to the single best tree after the first (a) -- the usual practice before topology tests; several trees sum
    their objectives.  One round is (b) then (a); the fit stops when a round raises the objective by less than tol, or after
    max_rounds.  The objective never falls: both halves take a step only if it does not lower it.

    The row-softmax fixes the scale of every row of Q (its off-diagonal entries sum to 1), so no direction of the model space
    rescales Q as a whole: branch lengths and Q are not confounded, and (a) and (b) do not chase one another along a ridge.

    grad_fn(blen [T][N-1][2], Q [4][4], pi [4]) -> (loglik [T], grad, curv): Context.trees_grad(want_curv=True) after set_model,
    or a restatement.  grad_model_fn(idx, blen [n][N-1][2], Q, pi, dirs [P][4][4]) -> (loglik [n], dtheta [n][P], dprior [n][4])
    for the trees idx: Context.trees_grad_model, or a restatement.

    Returns a dict: 'y_q' [4][4], 'y_station' [4], 'Q', 'pi', 'blen' [T][N-1][2] and 'loglik' [T] (every tree at its climbed
    lengths under the fitted model), 'fit_on', 'rounds', 'objective_start' (after the first (a): the objective under the
    starting model) and 'objective', 'history' (the objective after every half round, starting with objective_start),
    'grad_model' (the gradient of the fitted coordinates at the returned model and lengths), 'converged'."""
    from . import model as model_mod
    from . import modelfit
    fit = tuple(fit)
    if 'q' not in fit or any(f not in ('q', 'pi') for f in fit):
        raise ValueError("optimize_model: fit is ('q',) or ('q', 'pi'), not %r" % (fit,))
    fit_pi = 'pi' in fit
    b = np.array(blen, dtype=np.float64)
    if b.ndim == 2:
        b = b[None]
    T = b.shape[0]
    y_q = modelfit.unpack_q(modelfit.pack_q(y_q0))
    y_st = np.array(y_station0, dtype=np.float64).reshape(4)

    def model_of(yq, ys):
        return model_mod.get_Q(yq), model_mod.get_stationary_probs(ys).reshape(4)

    def lengths(bb, yq, ys):
        Q, pi = model_of(yq, ys)
        return optimize_branches(lambda x: grad_fn(x, Q, pi), child, bb, lo=lo, hi=hi, max_iter=branch_iter, gtol=gtol)

    out = lengths(b, y_q, y_st)
    b, ll = out['blen'], np.array(out['loglik'], dtype=np.float64)
    if fit_on is None:
        fit_on = [int(np.argmax(ll))]
    fit_on = [int(t) for t in np.atleast_1d(fit_on)]
    if not fit_on or min(fit_on) < 0 or max(fit_on) >= T:
        raise ValueError("optimize_model: fit_on names trees 0 .. %d, got %r" % (T - 1, fit_on))
    idx = np.array(fit_on)

    def value(v, bb):
        """the objective at model coordinates v and lengths bb: its value, the trees' terms and the gradient in v"""
        yq = modelfit.unpack_q(v[:12])
        ys = v[12:] if fit_pi else y_st
        Q, pi = model_of(yq, ys)
        l, dth, dpr = grad_model_fn(idx, bb[idx], Q, pi, modelfit.q_directions(yq))
        l = np.array(l, dtype=np.float64)
        g = np.asarray(dth, dtype=np.float64).sum(axis=0)
        if fit_pi:
            g = np.concatenate([g, modelfit.chain_prior(np.asarray(dpr, dtype=np.float64).sum(axis=0), ys)])
        return float(np.sum(l)), l, g

    def coords():
        return np.concatenate([modelfit.pack_q(y_q)] + ([y_st] if fit_pi else []))

    # Every recorded objective is value() at the point that is kept: optimize_branches records, of two log-likelihoods it cannot
    # tell apart, the larger, which need not be the value at the lengths it returns.
    obj, l_cur, gm = value(coords(), b)
    ll[idx] = l_cur
    start, history, rounds, converged = obj, [obj], 0, False
    for _ in range(max_rounds):
        v, f_b, _, _, _ = _climb_bfgs(lambda x: value(x, b)[::2], coords(), gtol)      # (b): starts at obj, returns its best point
        if f_b >= obj:                                      # taken only if it does not lower the objective
            y_q = modelfit.unpack_q(v[:12])
            if fit_pi:
                y_st = v[12:].copy()
        f_b, l_cur, gm = value(coords(), b)
        history.append(f_b)
        out = lengths(b, y_q, y_st)                         # (a)
        new, l_new, g_new = value(coords(), out['blen'])
        if new >= f_b:                                      # ... and so is (a)
            b, ll, l_cur, gm = out['blen'], np.array(out['loglik'], dtype=np.float64), l_new, g_new
        else:                                               # the lengths stay; every tree's value is that of its start under this model
            ll, new = np.array(out['history'][0], dtype=np.float64), f_b
        ll[idx] = l_cur
        history.append(new)
        rounds += 1
        rise, obj = new - obj, new
        if rise < tol:
            converged = True
            break
    Q, pi = model_of(y_q, y_st)
    return {'y_q': y_q, 'y_station': y_st, 'Q': Q, 'pi': pi, 'blen': b, 'loglik': ll, 'fit_on': fit_on, 'rounds': rounds,
            'objective_start': start, 'objective': obj, 'history': np.array(history), 'grad_model': gm, 'converged': converged,
            'branches': out}
