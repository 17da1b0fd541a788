"""Among-site rate variation for scoring explicit trees: the discrete Gamma model of Yang (1994, J. Mol.
Evol. 39:306-314), a proportion of invariant sites as a category of rate 0, and what a fitted mixture says about every site.

NumPy and the standard library only: the regularised incomplete gamma function is computed here (series below its mean,
continued fraction above it) and inverted by a safeguarded Newton iteration on log x.

    rates, weights = rate_model(alpha=0.5, C=4, pinv=0.1)
    loglik, cats = ctx.trees_loglik_rates(child, blen, rates, weights, want_cats=True)
    mean_rate, post = site_rates(cats, rates, weights)
"""
import math

import numpy as np

MAX_CATS = 16                                              # PT2_MAX_CATS of the C ABI
_EPS = 2.0 ** -53


def _gamma_series(a, x):
    """P(a, x) = x^a e^-x / Gamma(a + 1) * sum_n x^n / ((a+1) ... (a+n)): converges fast for x < a + 1"""
    term = total = 1.0
    n = a
    for _ in range(100000):
        n += 1.0
        term *= x / n
        total += term
        if term < total * _EPS:
            break
    return total * math.exp(a * math.log(x) - x - math.lgamma(a + 1.0))


def _gamma_cfrac(a, x):
    """Q(a, x) = 1 - P(a, x) by the continued fraction x + 1 - a - 1 (1 - a) / (x + 3 - a - ...) (modified Lentz): for x >= a + 1"""
    tiny = 1e-300
    b = x + 1.0 - a
    c = 1.0 / tiny
    d = 1.0 / b
    h = d
    for i in range(1, 100000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        if abs(d) < tiny:
            d = tiny
        c = b + an / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 2 * _EPS:
            break
    return h * math.exp(a * math.log(x) - x - math.lgamma(a))


def gamma_p(a, x):
    """The regularised lower incomplete gamma function P(a, x), a > 0, x >= 0."""
    a, x = float(a), float(x)
    if not a > 0.0 or not x >= 0.0:
        raise ValueError("gamma_p needs a > 0 and x >= 0 (a=%r, x=%r)" % (a, x))
    if x == 0.0:
        return 0.0
    if math.isinf(x):
        return 1.0
    return _gamma_series(a, x) if x < a + 1.0 else 1.0 - _gamma_cfrac(a, x)


def gamma_p_inv(a, p):
    """x with P(a, x) = p, 0 <= p < 1.  Newton on t = log x (the unknown spans hundreds of orders of magnitude at small a, and the
    relative error of x is the absolute error of t), kept inside a bracket that every evaluation tightens; a step that leaves
    the bracket is replaced by its midpoint."""
    a, p = float(a), float(p)
    if not a > 0.0 or not 0.0 <= p < 1.0:
        raise ValueError("gamma_p_inv needs a > 0 and 0 <= p < 1 (a=%r, p=%r)" % (a, p))
    if p == 0.0:
        return 0.0
    lga = math.lgamma(a)
    # starting points: the first term of the series (exact as x -> 0), and Wilson-Hilferty's cube for the bulk
    t = (math.log(p) + math.lgamma(a + 1.0)) / a
    if a >= 1.0:
        wh = 1.0 - 1.0 / (9.0 * a) + _normal_quantile(p) / (3.0 * math.sqrt(a))
        if wh > 0.05:
            t = math.log(a) + 3.0 * math.log(wh)
    lo, hi = -math.inf, math.inf
    for _ in range(200):
        x = math.exp(t)
        f = gamma_p(a, x) - p
        if f > 0.0:
            hi = t
        elif f < 0.0:
            lo = t
        else:
            return x
        slope = math.exp(a * t - x - lga)                  # dP/dt = x * density(x)
        step = f / slope if slope > 0.0 else math.inf
        new = t - step
        if not lo < new < hi:
            if math.isinf(lo):
                new = t - max(1.0, abs(t))                  # no lower end yet: walk down geometrically in x
            elif math.isinf(hi):
                new = t + max(1.0, abs(t))
            else:
                new = 0.5 * (lo + hi)
        if abs(new - t) <= 4 * _EPS * max(1.0, abs(t)) or hi - lo <= 4 * _EPS * max(1.0, abs(t)):
            return math.exp(new)
        t = new
    return math.exp(t)


def _normal_quantile(p):
    """a rough standard normal quantile (Abramowitz & Stegun 26.2.23, |error| < 4.5e-4): a starting point only"""
    q = p if p < 0.5 else 1.0 - p
    s = math.sqrt(-2.0 * math.log(q))
    z = s - (2.515517 + 0.802853 * s + 0.010328 * s * s) / (1.0 + 1.432788 * s + 0.189269 * s * s + 0.001308 * s ** 3)
    return -z if p < 0.5 else z


def discrete_gamma(alpha, C, kind='mean'):
    """C ascending rates of mean 1, each of probability 1/C, standing for a Gamma(alpha, alpha) distribution of rates (Yang 1994).
    The cut points are the quantiles q_k = P^-1(alpha, k / C) of the standard Gamma(alpha).  kind='mean': the mean rate of every
    class, C [P(alpha + 1, q_{k+1}) - P(alpha + 1, q_k)]; kind='median': the class medians P^-1(alpha, (2k + 1) / 2C) / alpha,
    rescaled to mean 1.  C = 1 is the single rate 1.0 exactly."""
    alpha, C = float(alpha), int(C)
    if not (alpha > 0.0 and math.isfinite(alpha)):
        raise ValueError("discrete_gamma needs a finite alpha > 0 (alpha=%r)" % alpha)
    if C < 1:
        raise ValueError("discrete_gamma needs C >= 1 (C=%r)" % C)
    if kind not in ('mean', 'median'):
        raise ValueError("kind is 'mean' or 'median', not %r" % (kind,))
    if C == 1:
        return np.array([1.0])
    if kind == 'median':
        r = np.array([gamma_p_inv(alpha, (2 * k + 1) / (2.0 * C)) / alpha for k in range(C)])
        return r * (C / r.sum())
    cut = [0.0] + [gamma_p(alpha + 1.0, gamma_p_inv(alpha, k / float(C))) for k in range(1, C)] + [1.0]
    return np.array([C * (cut[k + 1] - cut[k]) for k in range(C)])


def rate_model(alpha=None, C=4, pinv=0.0, keep_invariant=False):
    """(rates, weights) of a rate mixture for Context.trees_loglik_rates: C discrete Gamma categories of shape alpha (alpha None:
    the single rate 1), each of weight (1 - pinv) / C, and with pinv > 0 an invariant class first: rate 0, weight pinv.

    The rates of the variable sites are NOT rescaled by 1 / (1 - pinv): their mean stays 1 and the mean rate over all sites is
    1 - pinv, so a branch length counts substitutions per VARIABLE site -- the convention of PAML and PhyML, and the one under
    which a tree inferred by them under +I+G carries its branch lengths.  keep_invariant: the invariant class is there at
    pinv = 0 too (weight 0: an ordinary category), so that a fit of pinv keeps one layout."""
    pinv = float(pinv)
    if not 0.0 <= pinv < 1.0:
        raise ValueError("rate_model needs 0 <= pinv < 1 (pinv=%r)" % pinv)
    gam = np.array([1.0]) if alpha is None else discrete_gamma(alpha, C)
    w = np.full(gam.size, (1.0 - pinv) / gam.size)
    if pinv > 0.0 or keep_invariant:
        gam, w = np.concatenate([[0.0], gam]), np.concatenate([[pinv], w])
    if gam.size > MAX_CATS:
        raise ValueError("%d rate categories; at most %d" % (gam.size, MAX_CATS))
    return gam, w


JAC_STEP = 1e-4            # the step in log alpha of rate_model_jacobian's central difference


def rate_model_jacobian(alpha, C=4, pinv=0.0, keep_invariant=False):
    """(d rates / d alpha, d weights / d pinv) in rate_model's layout for the same arguments (the invariant class first when
    pinv > 0 or keep_invariant).  d weights / d pinv is exact: +1 for the invariant class, -1 / C for every other.  d rates /
    d alpha is the central difference of discrete_gamma in log alpha, (r(alpha e^h) - r(alpha e^-h)) / (2 h alpha) with h =
    JAC_STEP = 1e-4: the truncation term is of the order h^2 = 1e-8 of the rates' size and the rounding of discrete_gamma
    (about 1e-14) enters as 1e-14 / h = 1e-10; the invariant class has derivative 0."""
    alpha, C, pinv = float(alpha), int(C), float(pinv)
    if not 0.0 <= pinv < 1.0:
        raise ValueError("rate_model_jacobian needs 0 <= pinv < 1 (pinv=%r)" % pinv)
    up, dn = discrete_gamma(alpha * math.exp(JAC_STEP), C), discrete_gamma(alpha * math.exp(-JAC_STEP), C)
    dr = (up - dn) / (2.0 * JAC_STEP * alpha)
    dw = np.full(C, -1.0 / C)
    if pinv > 0.0 or keep_invariant:
        dr, dw = np.concatenate([[0.0], dr]), np.concatenate([[1.0], dw])
    return dr, dw


def chain(drate, dweight, jac):
    """(d loglik / d alpha, d loglik / d pinv) from Context.trees_grad_rates' drate and dweight [..., C] and rate_model_jacobian's
    pair, each [C] or [..., C] (one Jacobian per tree): the sums over the categories."""
    dr, dw = np.asarray(jac[0], dtype=np.float64), np.asarray(jac[1], dtype=np.float64)
    return (np.asarray(drate, dtype=np.float64) * dr).sum(axis=-1), (np.asarray(dweight, dtype=np.float64) * dw).sum(axis=-1)


def parse_spec(spec):
    """'gamma:ALPHA:C[:PINV]' (runner.py --score_rates) -> {'spec', 'rates', 'weights', 'alpha', 'C', 'pinv'}; ValueError on
    anything else."""
    parts = str(spec).split(':')
    if parts[0] != 'gamma' or len(parts) not in (3, 4):
        raise ValueError("a rate model is gamma:ALPHA:C or gamma:ALPHA:C:PINV, not %r" % (spec,))
    try:
        alpha, C = float(parts[1]), int(parts[2])
        pinv = float(parts[3]) if len(parts) == 4 else 0.0
    except ValueError:
        raise ValueError("a rate model is gamma:ALPHA:C or gamma:ALPHA:C:PINV with numbers, not %r" % (spec,)) from None
    rates, weights = rate_model(alpha, C, pinv)
    return {'spec': str(spec), 'rates': rates, 'weights': weights, 'alpha': alpha, 'C': C, 'pinv': pinv}


def site_rates(cat_lik, rates, weights):
    """What the mixture says about every site (empirical Bayes): cat_lik [..., C, S] are the categories' factors
    (trees_loglik_rates with want_cats).  Returns (mean_rate [..., S], post [..., C, S]): post[c] = weights[c] cat_lik[c] /
    sum_c weights[c] cat_lik[c], the posterior probability of category c at the site, and mean_rate = sum_c post[c] rates[c].
    A site of likelihood zero in every category has no posterior: NaN."""
    f = np.asarray(cat_lik, dtype=np.float64)
    r, w = np.asarray(rates, dtype=np.float64).reshape(-1), np.asarray(weights, dtype=np.float64).reshape(-1)
    if f.ndim < 2 or f.shape[-2] != r.size or w.size != r.size:
        raise ValueError("cat_lik must be [..., C, S] with C = len(rates) = len(weights), got %r for C = %d, %d" % (f.shape, r.size, w.size))
    joint = f * w[:, None]
    with np.errstate(invalid='ignore', divide='ignore'):
        post = joint / joint.sum(axis=-2, keepdims=True)
    return (post * r[:, None]).sum(axis=-2), post
