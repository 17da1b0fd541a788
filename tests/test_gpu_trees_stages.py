"""The nine scored-tree-set calls on ONE context.  They share one event pair and the stages of the driver,
so the only new way for one call to disturb another is through those: every output of every call, and its n_launches and units,
is held bit for bit to the same call on a fresh context -- in two interleaved orders, and after a call was refused (before anything
was queued, and by the range of the matrix exponential).

Shapes: N = 4 and 6 taxa; S = 130 sites under a site tile of 64 (three tiles, the last wave ragged); T = 5 trees under
PHYLO_TREES_CHUNK = 2 (three chunks, the last one short); C = 2 categories, one mixture for all trees and one per tree; coded and
generic leaves."""
import numpy as np
import pytest

from phylo_amd import _ffi
from test_gpu_trees_loglik import alignment, bits, gtr_Q, make_ctx, random_trees

pytestmark = pytest.mark.gpu
S, T, CHUNK, TILE = 130, 5, 2, 64
PRIOR = np.array([0.1, 0.2, 0.3, 0.4])
RATES = np.array([0.25, 1.75])
WEIGHTS = np.array([0.4, 0.6])
RATES_T = RATES[None, :] * (1.0 + 0.1 * np.arange(T))[:, None]          # per tree: [T][C]
WEIGHTS_T = np.stack([np.array([0.3 + 0.05 * t, 0.7 - 0.05 * t]) for t in range(T)])
DIRS = np.random.default_rng(3).normal(size=(2, 4, 4))


def calls(child, blen):
    """name -> the call on a context, every output asked for; shared and per-tree mixtures alternate over the rates calls"""
    return {
        'loglik': lambda c: c.trees_loglik(child, blen, prior=PRIOR, want_sites=True),
        'loglik_rates': lambda c: c.trees_loglik_rates(child, blen, RATES, WEIGHTS, prior=PRIOR, want_sites=True, want_cats=True),
        'grad': lambda c: c.trees_grad(child, blen, prior=PRIOR, want_curv=True),
        'grad_rates': lambda c: c.trees_grad_rates(child, blen, RATES_T, WEIGHTS_T, prior=PRIOR, want_curv=True, want_params=True),
        'grad_model': lambda c: c.trees_grad_model(child, blen, DIRS, prior=PRIOR, want_grad=True, want_prior=True),
        'ancestral': lambda c: c.trees_ancestral(child, blen, prior=PRIOR, want_post=True, want_state=True, want_pmax=True),
        'ancestral_rates': lambda c: c.trees_ancestral_rates(child, blen, RATES, WEIGHTS, prior=PRIOR, want_post=True, want_state=True,
                                                             want_pmax=True, want_catpost=True, want_siterate=True),
        'nni': lambda c: c.trees_nni(child, blen),                       # the model's own prior: the pointer the kernels read changes
        'nni_rates': lambda c: c.trees_nni_rates(child, blen, RATES_T, WEIGHTS_T, prior=PRIOR),
    }


def run(call, ctx):
    out = call(ctx)
    out = out if isinstance(out, tuple) else (out,)
    st = ctx.last_trees_stats
    return out, (st['n_launches'], st['units'])


def same(got, want, what):
    (out, st), (rout, rst) = got, want
    assert st == rst, (what, st, rst)
    assert len(out) == len(rout), what
    for k, (a, b) in enumerate(zip(out, rout)):
        if a.dtype == np.uint8:
            np.testing.assert_array_equal(a, b, err_msg="%s: output %d" % (what, k))
        else:
            np.testing.assert_array_equal(bits(a), bits(b), err_msg="%s: output %d" % (what, k))


@pytest.mark.parametrize("generic", [False, True], ids=['coded', 'generic'])
@pytest.mark.parametrize("N", [4, 6])
def test_nine_calls_share_one_context(N, generic, monkeypatch):
    monkeypatch.setenv('PHYLO_TREES_CHUNK', str(CHUNK))                   # read when a context is created
    g = alignment(N, S, 300 + N, gaps=True, generic=generic)
    Q = gtr_Q()
    child, blen = random_trees(N, 17 + N, T)
    todo = calls(child, blen)
    names = list(todo)
    fresh = {}
    for name in names:                                                    # every call on a context of its own
        with make_ctx(g, Q, tile=TILE) as ctx:
            assert ctx.site_tile() == TILE and -(-S // TILE) == 3
            fresh[name] = run(todo[name], ctx)
    n_chunks = -(-T // CHUNK)
    assert fresh['loglik'][1][0] == n_chunks * (3 if generic else 4)      # three chunks, the last one of one tree
    assert fresh['nni'][1][0] == n_chunks * (4 if generic else 5)
    # two interleaved orders: plain and rates calls alternate; the second round runs backwards from the middle
    first = ['grad_rates', 'loglik', 'ancestral_rates', 'nni', 'loglik_rates', 'grad_model', 'nni_rates', 'ancestral', 'grad']
    second = first[4::-1] + first[:4:-1]
    assert sorted(first) == sorted(names) == sorted(second) and first != second
    nan_b = blen.copy()
    nan_b[3, 1, 0] = np.nan                                               # tree 3 of 5: refused before anything is queued
    long_b = blen.copy()
    long_b[3, 1, 0] = 1e100                                               # refused by the range of the matrix exponential
    with make_ctx(g, Q, tile=TILE) as ctx:
        for rnd, order in enumerate((first, second)):
            for name in order:
                same(run(todo[name], ctx), fresh[name], "round %d, %s on the shared context" % (rnd + 1, name))
        for bad, word in ((nan_b, 'not a finite number'), (long_b, 'limit of the matrix exponential')):
            refused = calls(child, bad)
            for k, name in enumerate(names):
                with pytest.raises(_ffi.PhyloError) as e:
                    refused[name](ctx)
                assert 'tree 3, row 1' in str(e.value) and word in str(e.value), (name, str(e.value))
                after = names[(k + 4) % len(names)]                       # the next call is another one of the family
                same(run(todo[after], ctx), fresh[after], "%s after %s was refused (%s)" % (after, name, word))
