"""phylo_trees_loglik_rates on the device: sets of trees under a mixture of site rates.  The contract is
replayed bit for bit -- every category's factors are the site factors of phylo_trees_loglik on the scaled tree, the site values
are tests/rates_ref.py's chain over them --, the sum is held to the site-product bound and to the CPU oracle, degenerate
mixtures carry the plain call's bits; place, company, chunks and the optional outputs change nothing; refusals queue nothing;
runner.py --score_rates.

Every test here needs Context.trees_loglik_rates: AttributeError without it."""
import glob
import json
import math
import os
import subprocess
import sys
import tempfile

import mpmath as mp
import numpy as np
import pytest

import rates_ref
import site_product_ref as SP
from oracle import cpu_ref as O
from phylo_amd import _ffi, model
from phylo_amd import rates as R
from phylo_amd import treepost as TP
from phylo_amd.datasets import load_dataset, synthetic_alignment
from trees_cases import balanced_rows, caterpillar_rows, random_rows, rows_to_nodes

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PI = np.full(4, 0.25)
PRIOR = np.array([0.1, 0.2, 0.3, 0.4])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def gtr_Q(seed=7):
    return O.get_Q(np.random.default_rng(seed).normal(size=(4, 4)))


def make_ctx(g, Q, jc=False, pi=PI, tile=None):
    N, S, _ = g.shape
    ctx = _ffi.Context(4, N, S)
    if tile:
        ctx.set_site_tile(tile)
    ctx.set_leaves(g)
    ctx.set_model(Q, pi, np.full(N - 1, 10.0), np.full(N - 1, 10.0), jc69_closed_form=jc)
    return ctx


def alignment(N, S, seed, gaps=False, generic=False):
    g = synthetic_alignment(N, S, seed=seed)['genome'].copy()
    rng = np.random.default_rng(seed + 1)
    if gaps:
        g[rng.random((N, S)) < 0.15] = 1.0
    if generic:
        g[rng.integers(0, N), rng.integers(0, S)] = [0.5, 0.25, 0.0, 1.0]      # one row that is no indicator: no codes at all
    return g


def trees(N, seed, n, shape=None):
    """n trees: random topologies, or one shape with the leaves relabelled; lengths drawn anew for every tree"""
    rng = np.random.default_rng(seed)
    child, blen = [], []
    for _ in range(n):
        if shape is None:
            c, b = random_rows(N, rng)
        else:
            c, b = shape(N, rng)
            perm = rng.permutation(N)
            c = np.where(c < N, perm[np.minimum(c, N - 1)], c).astype(np.int32)
        child.append(c)
        blen.append(b)
    return np.array(child), np.array(blen)


MODELS = {
    'C1': (np.array([1.3]), np.array([0.9])),
    'C2': R.rate_model(0.5, 2),
    'C4': R.rate_model(0.5, 4),
    'C5-invariant': R.rate_model(0.5, 4, 0.2),              # a rate-0 category of weight 0.2
    'C3-weight0': (np.array([0.2, 1.0, 2.5]), np.array([0.5, 0.0, 0.5])),
}


def case(N, S, **kw):
    return dict(N=N, S=S, **kw)


CASES = {
    'N2': case(2, 130), 'N12': case(12, 130),
    'S1': case(12, 1), 'S64': case(12, 64), 'S65': case(12, 65),
    'S130-tile64': case(12, 130, tile=64),
    'caterpillar-N20-S300': case(20, 300, shape=caterpillar_rows),
    'balanced-N16': case(16, 130, shape=balanced_rows),
    'gaps': case(12, 130, gaps=True),
    'generic': case(12, 130, generic=True),
    'generic-caterpillar-N20-S300': case(20, 300, shape=caterpillar_rows, generic=True, gaps=True),
    'jc69': case(12, 130, jc=True),
}
RUNS = [(name, 'C4') for name in CASES] + [('N12', m) for m in MODELS if m != 'C4'] + \
    [('caterpillar-N20-S300', 'C5-invariant'), ('balanced-N16', 'C3-weight0'), ('gaps', 'C5-invariant')]


# ---- 1. composition and the sum ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mname", RUNS, ids=['%s-%s' % r for r in RUNS])
def test_composition_bit_for_bit_and_the_sum(name, mname):
    kw = CASES[name]
    N, S, jc, n = kw['N'], kw['S'], kw.get('jc', False), 3
    rates, weights = MODELS[mname]
    C = rates.size
    g = alignment(N, S, 100 + N + S, kw.get('gaps', False), kw.get('generic', False))
    Q = O.jc_Q() if jc else gtr_Q()
    child, blen = trees(N, 5, n, kw.get('shape'))
    depths = [_ffi.debug_tree_schedule(c, b)[1] for c, b in zip(child, blen)]
    if 'caterpillar' in name:
        assert max(depths) == 1 and S > 256 and S % 256 != 0             # four site steps per pass, a partial last pass
    if 'balanced' in name:
        assert min(depths) == 4                                           # two site steps per pass
    with make_ctx(g, Q, jc=jc, tile=kw.get('tile')) as ctx:
        tile = ctx.site_tile()
        if 'tile' in kw:
            assert tile == kw['tile'] and (S + tile - 1) // tile == 3
        ll, sites, cats = ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR, want_sites=True, want_cats=True)
        st = ctx.last_trees_stats
        assert st['units'] == n * S * (N - 1) * C and st['n_launches'] >= 3 and st['sweep_ms'] > 0
        assert ll.shape == (n,) and sites.shape == (n, S) and cats.shape == (n, C, S)
        np.testing.assert_array_equal(bits(ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR)), bits(ll),
                                      err_msg="no output asked for")
        # every category: the site factors of the plain call on the scaled trees
        for c in range(C):
            _, f = ctx.trees_loglik(child, rates[c] * blen, prior=PRIOR, want_sites=True)
            np.testing.assert_array_equal(bits(cats[:, c, :]), bits(f), err_msg="category %d" % c)
        # the site values: the chain over those factors
        ref = np.array([rates_ref.mix(weights, cats[t]) for t in range(n)])
        np.testing.assert_array_equal(bits(sites), bits(ref), err_msg="the mixing chain")
        assert np.isfinite(ll).all() and (sites > 0).all()
        # the sum: within the site-product bound of the exact sum of logs of the site values ...
        for t in range(n):
            exact, bound = SP.row_bound(sites[t], tile)
            err = float(abs(mp.mpf(float(ll[t])) - exact))
            print("%s %s tree %d: loglik %.17g |err| %.3g bound %.3g" % (name, mname, t, ll[t], err, bound))
            assert err <= bound, (t, ll[t], err, bound)
        # ... and the CPU oracle's sum_s log sum_c w_c f_c on the scaled trees
        for t in range(n):
            left, right, bl, br = rows_to_nodes(child[t], blen[t])
            mixed = np.zeros(S)
            for c in range(C):
                _, root = O.tree_loglik(Q, PRIOR, 2 * N - 1, left, right, rates[c] * bl, rates[c] * br, 2 * N - 2, g)
                mixed += weights[c] * (root @ PRIOR)
            want = float(np.sum(np.log(mixed)))
            print("%s %s tree %d: oracle %.17g rel %.3g" % (name, mname, t, want, abs(ll[t] - want) / abs(want)))
            assert ll[t] == pytest.approx(want, rel=1e-12), (t, ll[t], want)


# ---- 2. degenerate mixtures carry the plain call's bits -------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=['coded', 'generic'])
def test_degenerate_mixtures_are_the_plain_call(generic):
    N, S = 12, 130
    g = alignment(N, S, 51, gaps=True, generic=generic)
    child, blen = trees(N, 6, 5)
    with make_ctx(g, gtr_Q()) as ctx:
        plain, f = ctx.trees_loglik(child, blen, prior=PRIOR, want_sites=True)
        for rates, weights in (([1.0], [1.0]), ([1.0, 1.0], [0.5, 0.5])):
            ll, sites = ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR, want_sites=True)
            np.testing.assert_array_equal(bits(ll), bits(plain), err_msg=str(rates))
            np.testing.assert_array_equal(bits(sites), bits(f), err_msg=str(rates))
        ll = ctx.trees_loglik_rates(child, blen, [0.7, 3.0], [1.0, 0.0], prior=PRIOR)
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, 0.7 * blen, prior=PRIOR)))


# ---- 3. invariance and isolation --------------------------------------------------------------------------------------------
def test_place_company_and_the_optional_outputs():
    N, S, n = 12, 130, 7
    g = alignment(N, S, 52, gaps=True)
    child, blen = trees(N, 7, n)
    rates, weights = MODELS['C5-invariant']
    with make_ctx(g, gtr_Q()) as ctx:
        ll, sites, cats = ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR, want_sites=True, want_cats=True)
        only = ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR)
        assert isinstance(only, np.ndarray) and only.shape == (n,)
        np.testing.assert_array_equal(bits(only), bits(ll))
        l2, s2 = ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR, want_sites=True)
        l3, c3 = ctx.trees_loglik_rates(child, blen, rates, weights, prior=PRIOR, want_cats=True)
        np.testing.assert_array_equal(bits(l2), bits(ll))
        np.testing.assert_array_equal(bits(l3), bits(ll))
        np.testing.assert_array_equal(bits(s2), bits(sites))
        np.testing.assert_array_equal(bits(c3), bits(cats))
        rl, rs, rc = ctx.trees_loglik_rates(child[::-1], blen[::-1], rates, weights, prior=PRIOR, want_sites=True, want_cats=True)
        np.testing.assert_array_equal(bits(rl[::-1]), bits(ll))         # a tree's bits do not depend on its place in the call
        np.testing.assert_array_equal(bits(rs[::-1]), bits(sites))
        np.testing.assert_array_equal(bits(rc[::-1]), bits(cats))
        ol, oc = ctx.trees_loglik_rates(child[3], blen[3], rates, weights, prior=PRIOR, want_cats=True)   # ... nor on its company
        assert ol.shape == (1,) and bits(ol)[0] == bits(ll)[3]
        np.testing.assert_array_equal(bits(oc[0]), bits(cats[3]))


def test_prior_none_is_the_models_pi():
    g = alignment(7, 70, 3, gaps=True)
    pi = np.array([0.4, 0.3, 0.2, 0.1])
    child, blen = trees(7, 9, 5)
    rates, weights = MODELS['C4']
    with make_ctx(g, gtr_Q(), pi=pi) as ctx:
        a = ctx.trees_loglik_rates(child, blen, rates, weights, want_sites=True, want_cats=True)
        b = ctx.trees_loglik_rates(child, blen, rates, weights, prior=pi, want_sites=True, want_cats=True)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(bits(x), bits(y))
        assert not np.array_equal(a[0], ctx.trees_loglik_rates(child, blen, rates, weights, prior=PI))


def test_a_site_of_likelihood_zero_in_every_category():
    N, S = 5, 70
    g = alignment(N, S, 22, generic=True)
    g[2, 66] = 0.0                                                       # a zero leaf row kills the site in every tree and category
    child, blen = trees(N, 4, 3)
    rates, weights = MODELS['C5-invariant']
    with make_ctx(g, gtr_Q()) as ctx:
        ll, sites, cats = ctx.trees_loglik_rates(child, blen, rates, weights, prior=PI, want_sites=True, want_cats=True)
        assert (ll == -np.inf).all()
        assert (sites[:, 66] == 0).all() and (cats[:, :, 66] == 0).all() and (np.delete(sites, 66, axis=1) > 0).all()


CHUNK_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from test_gpu_trees_rates import MODELS, alignment, gtr_Q, make_ctx, trees
g = alignment(12, 130, 31, gaps=True)
child, blen = trees(12, 6, 7)
rates, weights = MODELS['C5-invariant']
with make_ctx(g, gtr_Q()) as ctx:
    ll, sites, cats = ctx.trees_loglik_rates(child, blen, rates, weights, want_sites=True, want_cats=True)
    np.savez(sys.argv[1], ll=ll, sites=sites, cats=cats, launches=ctx.last_trees_stats['n_launches'])
"""


def test_chunks_give_the_bits_of_one_chunk():
    """PHYLO_TREES_CHUNK is read when the context is created: a fresh process per setting"""
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for chunk in ('0', '3'):
            out = os.path.join(tmp, 'c%s.npz' % chunk)
            env = dict(os.environ, PHYLO_TREES_CHUNK=chunk)
            p = subprocess.run([sys.executable, '-c', CHUNK_SCRIPT % (ROOT, os.path.join(ROOT, 'tests')), out], env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
            assert p.returncode == 0, p.stdout.decode()[-2000:]
            got[chunk] = dict(np.load(out))
    assert int(got['0']['launches']) == 4 and int(got['3']['launches']) == 4 * 3        # 7 trees in chunks of 3
    for key in ('ll', 'sites', 'cats'):
        np.testing.assert_array_equal(bits(got['3'][key]), bits(got['0'][key]), err_msg=key)


def test_the_sweep_and_a_pending_summary_are_left_alone():
    g = load_dataset('primate_data')['genome'][:6, 100:170].copy()
    N, S, K, seed = 6, 70, 64, 5
    pi = np.array([[0.3, 0.2, 0.2, 0.3]])
    Q = model.get_Q(model.init_y_q())
    lam = np.linspace(5.0, 15.0, N - 1)
    rates, weights = MODELS['C5-invariant']
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, pi, lam, lam[::-1].copy())
        out = ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        grad = ctx.sweep_backward()
        ctx.sweep_async(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)      # score between a sweep and its pending reverse pass
        child, blen = TP.particle_trees(out['merges'], out['ancestors'], out['left_branches'], out['right_branches'], seed=seed)
        ll = ctx.trees_loglik_rates(child[:7], blen[:7], rates, weights)
        assert np.isfinite(ll).all()
        grad2 = ctx.sweep_backward()
        again = ctx.sweep_fetch()
        for key in ('log_weights', 'log_likelihood', 'left_branches', 'right_branches'):
            np.testing.assert_array_equal(bits(again[key]), bits(out[key]), err_msg=key)
        np.testing.assert_array_equal(again['ancestors'], out['ancestors'])
        assert bits(again['logZ']) == bits(out['logZ'])
        for key in ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q'):
            np.testing.assert_array_equal(bits(grad2[key]), bits(grad[key]), err_msg=key)
        tab = ctx.tree_summary()                                               # ... and a tree summary keeps its branch pass
        ctx.trees_loglik_rates(child[:3], blen[:3], rates, weights, want_cats=True)
        tb = ctx.tree_branches(tab)
        assert np.isfinite(tb['leaf_stats']).all()
        third = ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        np.testing.assert_array_equal(bits(third['log_weights']), bits(out['log_weights']))


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing():
    N, S = 5, 70
    g = alignment(N, S, 41)
    child, blen = trees(N, 8, 4)
    child[2] = np.array([[0, 1], [2, 3], [6, 4], [5, 7]], dtype=np.int32)
    rates, weights = MODELS['C4']
    with _ffi.Context(4, N, S) as ctx:
        with pytest.raises(_ffi.PhyloError) as e:
            ctx.trees_loglik_rates(child, blen, rates, weights)
        assert e.value.code == -6
        ctx.set_leaves(g)
        with pytest.raises(_ffi.PhyloError) as e:
            ctx.trees_loglik_rates(child, blen, rates, weights)
        assert e.value.code == -6
        ctx.set_model(gtr_Q(), PI, np.full(N - 1, 10.0), np.full(N - 1, 10.0))
        ref = ctx.trees_loglik_rates(child, blen, rates, weights, want_sites=True, want_cats=True)
        for c in range(4):                                                 # (the reference itself: the plain call's factors)
            np.testing.assert_array_equal(bits(ref[2][:, c]), bits(ctx.trees_loglik(child, rates[c] * blen, want_sites=True)[1]))

        def refused(c, b, r, w, *what):
            with pytest.raises(_ffi.PhyloError) as e:
                ctx.trees_loglik_rates(c, b, r, w)
            assert e.value.code == -1, str(e.value)
            for x in what:
                assert x in str(e.value), str(e.value)
            again = ctx.trees_loglik_rates(child, blen, rates, weights, want_sites=True, want_cats=True)    # a valid call still works
            for x, y in zip(again, ref):
                np.testing.assert_array_equal(bits(x), bits(y))

        refused(child, blen, [], [], 'C=0')
        refused(child, blen, np.ones(17), np.full(17, 1 / 17), 'C=17')
        for v in (-1e-9, np.nan, np.inf, -np.inf):
            r = rates.copy(); r[2] = v
            refused(child, blen, r, weights, 'rate', 'category 2')
            w = weights.copy(); w[1] = v
            refused(child, blen, rates, w, 'weight', 'category 1')
        b = blen.copy(); b[1, 3, 0] = 1e308
        refused(child, b, [0.5, 1.0, 10.0], [0.3, 0.3, 0.4], 'tree 1, row 3, category 2')     # rate * blen overflows
        c = child.copy(); c[2, 2] = [6, 0]
        refused(c, blen, rates, weights, 'tree 2, row 2', 'twice')
        b = blen.copy(); b[3, 1, 1] = -1.0
        refused(child, b, rates, weights, 'tree 3, row 1', '>= 0')
        with pytest.raises(_ffi.PhyloError) as e:
            ctx._check(ctx._lib.phylo_trees_loglik_rates(ctx._h, 0, None, None, 1, None, None, None, None, None, None, None))
        assert e.value.code == -1
        with pytest.raises(ValueError):
            ctx.trees_loglik_rates(child, blen, rates, weights[:3])
        with pytest.raises(ValueError):
            ctx.trees_loglik_rates(child[:, :3], blen[:, :3], rates, weights)


# ---- 5. the runner ----------------------------------------------------------------------------------------------------------
RUNNER_SCRIPT = r"""
import sys
sys.path.insert(0, %r)
import runner
from phylo_amd.datasets import load_dataset
from phylo_amd.vcsmc import VCSMC
args = runner.parse_args(sys.argv[1:])
d = load_dataset(args.dataset)
d = {'taxa': d['taxa'][:6], 'genome': d['genome'][:6].copy()}          # a 6-taxon slice
VCSMC(d, K=args.n_particles, args=args).train(epochs=args.num_epoch, batch_size=args.batch_size, learning_rate=args.learning_rate,
                                              memory_optimization=args.memory_optimization)
"""


def test_runner_score_rates():
    d = load_dataset('primate_data_wang')
    taxa, g = [str(t) for t in d['taxa'][:6]], d['genome'][:6].copy()
    N = len(taxa)
    child, blen = trees(N, 12, 3)
    newicks = [TP.rows_to_newick(c, b, taxa) for c, b in zip(child, blen)]
    argv = ['--dataset', 'primate_data_wang', '--n_particles', '16', '--num_epoch', '1', '--batch_size', '512', '--jcmodel', 'true',
            '--seed', '2', '--tree_summary', 'true', '--tree_branches', 'true']
    spec = 'gamma:0.5:4:0.1'
    rates, weights = R.rate_model(0.5, 4, 0.1)
    for extra in (['--score_rates', spec], []):
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, 'trees.nwk')
            with open(path, 'w') as f:
                f.write('\n'.join(newicks) + '\n')
            p = subprocess.run([sys.executable, '-c', RUNNER_SCRIPT % ROOT] + argv + ['--score_trees', path] + extra, cwd=tmp,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
            assert p.returncode == 0, p.stdout.decode()[-2000:]
            (res,) = glob.glob(os.path.join(tmp, 'results', '*', '*', '*', '*', 'tree_scores.json'))
            with open(res) as f:
                scores = json.load(f)
            with open(os.path.join(os.path.dirname(res), 'run_parameters.txt')) as f:
                params = f.read()
            with open(os.path.join(os.path.dirname(res), 'map.tre')) as f:
                mc, mb = TP.newick_to_rows(f.read(), taxa)
            mdl = scores['model']
            got = np.array([t['loglik'] for t in scores['trees']])
            with make_ctx(g, np.array(mdl['Q']), jc=True, pi=np.array(mdl['pi'])) as ctx:
                if extra:
                    assert scores['rates'] == {'spec': spec, 'rates': rates.tolist(), 'weights': weights.tolist()}
                    assert 'score_rates : ' + spec in params
                    ref = ctx.trees_loglik_rates(child, blen, rates, weights)
                    top = ctx.trees_loglik_rates(mc, mb, rates, weights)
                    assert not np.array_equal(ref, ctx.trees_loglik(child, blen))
                else:                                      # without the flag: the file and the parameters know nothing of it
                    assert list(scores) == ['model', 'trees', 'best', 'summary'] and 'score_rates' not in params
                    ref = ctx.trees_loglik(child, blen)
                    top = ctx.trees_loglik(mc, mb)
                assert got.shape == (3,) and np.isfinite(got).all()
                np.testing.assert_array_equal(bits(got), bits(ref))
                assert scores['best'] == int(np.argmax(ref))
                assert bits(scores['summary']['map']['loglik']) == bits(top)[0]        # every score of the file is under the model
                assert bits(scores['summary']['topologies'][0]['loglik']) == bits(top)[0]
                assert math.isfinite(scores['summary']['consensus_bl']['loglik'])
