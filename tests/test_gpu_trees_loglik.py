"""phylo_trees_loglik on the device: many explicit trees over the context's resident alignment, bit for
bit what phylo_tree_loglik and the C oracle give tree by tree; the reference's golden trees; per-site factors; the trees of a
sweep's final particles against the sweep's own log-likelihoods; chunking; refusals; runner.py --score_trees.

Every test here needs phylo_trees_loglik: on a tree without it, Context.trees_loglik raises AttributeError."""
import glob
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import cpu_ref as O
from phylo_amd import _ffi, model
from phylo_amd import treepost as TP
from phylo_amd.datasets import load_dataset, synthetic_alignment
from trees_cases import balanced_rows, caterpillar_rows, nodes_to_rows, random_rows, rows_to_nodes

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PI = np.full(4, 0.25)
T = 37


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


def one_by_one(ctx, g, Q, prior, child, blen, jc=False):
    """the same trees through phylo_tree_loglik (leaves uploaded per call) and through the C oracle"""
    N = g.shape[0]
    dev, ora, roots = [], [], []
    for c, b in zip(child, blen):
        left, right, bl, br = rows_to_nodes(c, b)
        ll, root = ctx.tree_loglik(left, right, bl, br, 2 * N - 2, g, prior)
        ll_c, _ = CO.tree_loglik(Q, prior, left, right, bl, br, 2 * N - 2, g, jc=jc)
        dev.append(ll)
        ora.append(ll_c)
        roots.append(root)
    return np.array(dev), np.array(ora), np.array(roots)


def alignment(N, S, seed, gaps=False, generic=False):
    g = synthetic_alignment(N, S, seed=seed)['genome'].copy()
    rng = np.random.default_rng(seed + 1)
    if gaps:
        g[rng.random((N, S)) < 0.15] = 1.0
    if generic:
        g[rng.integers(0, N), rng.integers(0, S)] = [0.5, 0.25, 0.0, 1.0]      # one row that is no indicator: no codes at all
    return g


def random_trees(N, seed, n=T):
    rng = np.random.default_rng(seed)
    rows = [random_rows(N, rng) for _ in range(n)]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])


def shaped_trees(make, N, seed, n=T):
    """one shape, the leaves relabelled and the lengths drawn anew for every tree"""
    rng = np.random.default_rng(seed)
    child, blen = [], []
    for _ in range(n):
        c, b = make(N, rng)
        perm = rng.permutation(N)
        c = np.where(c < N, perm[np.minimum(c, N - 1)], c).astype(np.int32)
        child.append(c)
        blen.append(b)
    return np.array(child), np.array(blen)


# ---- 1. the reference's golden trees ---------------------------------------------------------------------------------------
def test_reference_goldens_one_call_per_alignment(golden_dir):
    nodes = np.load(os.path.join(golden_dir, "csmc_nodes.npz"))
    cases = [str(t) for t in nodes['cases']]
    by_ctx = {}
    for tag in cases:
        dname, _, qname = tag.split('/')
        by_ctx.setdefault((dname, qname), []).append(tag)
    seen = 0
    for (dname, qname), tags in by_ctx.items():
        g, Q = nodes['genome/' + dname], nodes['Q/' + qname]
        N = g.shape[0]
        rows = [nodes_to_rows(nodes[t + '/left'], nodes[t + '/right'], nodes[t + '/bl'], nodes[t + '/br'], int(nodes[t + '/root']), N)
                for t in tags]
        with make_ctx(g, Q) as ctx:
            ll = ctx.trees_loglik(np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), prior=PI)
            for t, x in zip(tags, ll):
                assert x == pytest.approx(float(nodes[t + '/loglik']), rel=1e-12), t
                one, _ = ctx.tree_loglik(nodes[t + '/left'], nodes[t + '/right'], nodes[t + '/bl'], nodes[t + '/br'],
                                         int(nodes[t + '/root']), g, PI)
                ora, _ = CO.tree_loglik(Q, PI, nodes[t + '/left'], nodes[t + '/right'], nodes[t + '/bl'], nodes[t + '/br'],
                                        int(nodes[t + '/root']), g)
                assert bits(x) == bits(one) == bits(ora), (t, x, one, ora)
                seen += 1
    assert seen == len(cases) == 48


# ---- 2. random trees, bit for bit -----------------------------------------------------------------------------------------
def case(N, S, **kw):
    return dict(N=N, S=S, **kw)


CASES = {
    'N2': case(2, 130), 'N3': case(3, 130), 'N12': case(12, 130), 'N33': case(33, 130),
    'S1': case(12, 1), 'S63': case(12, 63), 'S64': case(12, 64), 'S65': case(12, 65),
    'S4100-tile2048': case(5, 4100, tile=2048),
    'S130-tile64': case(12, 130, tile=64),
    'gaps': case(12, 130, gaps=True), 'gaps-N33-jc': case(33, 65, gaps=True, jc=True),
    'generic': case(12, 130, generic=True), 'generic-N33-S4100': case(33, 4100, generic=True, gaps=True, n=5),
    'jc69': case(12, 130, jc=True),
    'caterpillar-N70': case(70, 64, shape=caterpillar_rows), 'balanced-N128': case(128, 64, shape=balanced_rows, gaps=True),
    'generic-balanced-N128': case(128, 64, shape=balanced_rows, generic=True, n=5),
}


@pytest.mark.parametrize("name", list(CASES))
def test_random_trees_bit_for_bit(name):
    kw = CASES[name]
    N, S, jc, n = kw['N'], kw['S'], kw.get('jc', False), kw.get('n', T)
    g = alignment(N, S, 100 + N + S, kw.get('gaps', False), kw.get('generic', False))
    Q = O.jc_Q() if jc else gtr_Q()
    prior = np.array([0.1, 0.2, 0.3, 0.4])
    child, blen = shaped_trees(kw['shape'], N, 5, n) if 'shape' in kw else random_trees(N, 5, n)
    if N > 2:
        assert (blen == 0).any()
    depths = [_ffi.debug_tree_schedule(c, b)[1] for c, b in zip(child, blen)]
    if name.startswith('caterpillar'):
        assert max(depths) == 1                                           # four site steps per pass
    if 'balanced' in name:
        assert min(depths) == 7                                           # the deepest stack of 128 taxa: two site steps per pass
    CO.set_site_tile(kw.get('tile', 0))                                   # the oracle takes the context's site tile
    try:
        with make_ctx(g, Q, jc=jc, tile=kw.get('tile')) as ctx:
            if 'tile' in kw:
                assert ctx.site_tile() == kw['tile'] and (S + kw['tile'] - 1) // kw['tile'] == (3 if S > 130 or kw['tile'] == 64 else 1)
            ll = ctx.trees_loglik(child, blen, prior=prior)
            st = ctx.last_trees_stats
            assert st['units'] == n * S * (N - 1) and st['n_launches'] >= 3 and st['sweep_ms'] > 0
            dev, ora, _ = one_by_one(ctx, g, Q, prior, child, blen, jc=jc)
            assert np.isfinite(ll).all()
            np.testing.assert_array_equal(bits(ll), bits(dev), err_msg="against phylo_tree_loglik")
            np.testing.assert_array_equal(bits(ll), bits(ora), err_msg="against the C oracle")
            rev = ctx.trees_loglik(child[::-1], blen[::-1], prior=prior)      # a tree's bits do not depend on its place in the call
            np.testing.assert_array_equal(bits(rev[::-1]), bits(ll))
            one = ctx.trees_loglik(child[3 % n], blen[3 % n], prior=prior)    # ... nor on its company
            assert one.shape == (1,) and bits(one)[0] == bits(ll)[3 % n]
    finally:
        CO.set_site_tile(0)


def test_prior_none_is_the_models_pi():
    g = alignment(7, 70, 3, gaps=True)
    pi = np.array([0.4, 0.3, 0.2, 0.1])
    child, blen = random_trees(7, 9, 5)
    with make_ctx(g, gtr_Q(), pi=pi) as ctx:
        np.testing.assert_array_equal(bits(ctx.trees_loglik(child, blen)), bits(ctx.trees_loglik(child, blen, prior=pi)))
        assert not np.array_equal(ctx.trees_loglik(child, blen), ctx.trees_loglik(child, blen, prior=PI))


# ---- 3. per-site factors --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=['coded', 'generic'])
def test_site_factors(generic):
    N, S = 12, 4100
    g = alignment(N, S, 21, gaps=True, generic=generic)
    Q, prior = gtr_Q(), np.array([0.1, 0.2, 0.3, 0.4])
    child, blen = random_trees(N, 2, 4)
    with make_ctx(g, Q) as ctx:
        ll, sites = ctx.trees_loglik(child, blen, prior=prior, want_sites=True)
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=prior)))
        dev, _, roots = one_by_one(ctx, g, Q, prior, child, blen)
        assert sites.shape == (4, S) and (sites > 0).all()
        np.testing.assert_allclose(sites, roots @ prior, rtol=1e-14, atol=0)


def test_a_site_of_likelihood_zero():
    N, S = 5, 70
    g = alignment(N, S, 22, generic=True)
    g[2, 66] = 0.0                                                       # a zero leaf row kills the site in every tree
    Q = gtr_Q()
    child, blen = random_trees(N, 4, 3)
    with make_ctx(g, Q) as ctx:
        ll, sites = ctx.trees_loglik(child, blen, prior=PI, want_sites=True)
        dev, ora, _ = one_by_one(ctx, g, Q, PI, child, blen)
        assert (ll == -np.inf).all() and (dev == -np.inf).all() and (ora == -np.inf).all()
        assert (sites[:, 66] == 0).all() and (np.delete(sites, 66, axis=1) > 0).all()


# ---- 4. end to end with the sweep -----------------------------------------------------------------------------------------
def test_particle_trees_of_a_sweep_and_the_sweep_is_left_alone():
    g = load_dataset('primate_data')['genome'][:6, 100:170].copy()
    N, S, K, seed = 6, 70, 64, 5
    pi = np.array([[0.3, 0.2, 0.2, 0.3]])
    Q = model.get_Q(model.init_y_q())
    lam = np.linspace(5.0, 15.0, N - 1)
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, pi, lam, lam[::-1].copy())
        out = ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        grad = ctx.sweep_backward()
        # score between a sweep and its pending reverse pass
        ctx.sweep_async(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        child, blen = TP.particle_trees(out['merges'], out['ancestors'], out['left_branches'], out['right_branches'], seed=seed)
        ll = ctx.trees_loglik(child, blen)
        grad2 = ctx.sweep_backward()
        again = ctx.sweep_fetch()
        ldf = sum(math.log(v) for v in range(2 * N - 3, 1, -2))
        # log_likelihood of the last rank event = the tree's log-likelihood - log (2N-3)!! + the reference's branch-length prior
        # term: COLUMN k of the sampled lengths of all rank events (the reference does not resample its branch tensors along the
        # ancestry), every one at the last rank event's rates.  A handful of roundings on either side: rel 1e-12.
        lam_l, lam_r = lam[N - 2], lam[::-1][N - 2]
        bprior = (-lam_l * out['left_branches'] + math.log(lam_l)).sum(axis=0) + (-lam_r * out['right_branches'] + math.log(lam_r)).sum(axis=0)
        np.testing.assert_allclose(ll - ldf + bprior, out['log_likelihood'][N - 2], rtol=1e-12, atol=0)
        for key in ('log_weights', 'log_likelihood', 'left_branches', 'right_branches'):
            np.testing.assert_array_equal(bits(again[key]), bits(out[key]), err_msg=key)
        np.testing.assert_array_equal(again['ancestors'], out['ancestors'])
        assert bits(again['logZ']) == bits(out['logZ'])
        for key in ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q'):
            np.testing.assert_array_equal(bits(grad2[key]), bits(grad[key]), err_msg=key)
        # ... and a tree summary made before the call still has its branch pass
        tab = ctx.tree_summary()
        ctx.trees_loglik(child[:3], blen[:3])
        tb = ctx.tree_branches(tab)
        assert np.isfinite(tb['leaf_stats']).all()
        third = ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        np.testing.assert_array_equal(bits(third['log_weights']), bits(out['log_weights']))


# ---- 5. chunking ----------------------------------------------------------------------------------------------------------
CHUNK_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from test_gpu_trees_loglik import alignment, gtr_Q, make_ctx, random_trees
g = alignment(12, 130, 31, gaps=True)
child, blen = random_trees(12, 6)
with make_ctx(g, gtr_Q()) as ctx:
    ll, sites = ctx.trees_loglik(child, blen, want_sites=True)
    np.savez(sys.argv[1], ll=ll, sites=sites, launches=ctx.last_trees_stats['n_launches'])
"""


def test_chunks_give_the_bits_of_one_chunk():
    """PHYLO_TREES_CHUNK is read when the context is created: a fresh process per setting"""
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for chunk in ('0', '5'):
            out = os.path.join(tmp, 'c%s.npz' % chunk)
            env = dict(os.environ, PHYLO_TREES_CHUNK=chunk)
            p = subprocess.run([sys.executable, '-c', CHUNK_SCRIPT % (ROOT, os.path.join(ROOT, 'tests')), out], env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
            assert p.returncode == 0, p.stdout.decode()[-2000:]
            got[chunk] = dict(np.load(out))
    assert int(got['0']['launches']) == 4 and int(got['5']['launches']) == 4 * 8       # 37 trees in chunks of 5
    np.testing.assert_array_equal(bits(got['5']['ll']), bits(got['0']['ll']))
    np.testing.assert_array_equal(bits(got['5']['sites']), bits(got['0']['sites']))


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing():
    N, S = 5, 70
    g = alignment(N, S, 41)
    child, blen = random_trees(N, 8, 4)
    good = np.array([[0, 1], [2, 3], [6, 4], [5, 7]], dtype=np.int32)
    child[2] = good
    with _ffi.Context(4, N, S) as ctx:
        with pytest.raises(_ffi.PhyloError) as e:
            ctx.trees_loglik(child, blen)
        assert e.value.code == -6
        ctx.set_leaves(g)
        with pytest.raises(_ffi.PhyloError) as e:
            ctx.trees_loglik(child, blen)
        assert e.value.code == -6
        ctx.set_model(gtr_Q(), PI, np.full(N - 1, 10.0), np.full(N - 1, 10.0))
        ref = ctx.trees_loglik(child, blen)

        def refused(c, b, row, what):
            with pytest.raises(_ffi.PhyloError) as e:
                ctx.trees_loglik(c, b)
            assert e.value.code == -1 and 'tree 2, row %d' % row in str(e.value) and what in str(e.value), str(e.value)
            np.testing.assert_array_equal(bits(ctx.trees_loglik(child, blen)), bits(ref))     # a valid call still works

        c = child.copy(); c[2, 2] = [6, 0]
        refused(c, blen, 2, 'twice')                                     # a leaf used twice
        c = child.copy(); c[2, 1] = [2, 2]
        refused(c, blen, 1, 'twice')                                     # a taxon missing
        c = child.copy(); c[2, 0] = [0, 6]; c[2, 2] = [1, 4]
        refused(c, blen, 0, 'earlier row')                               # a child from a later row
        c = child.copy(); c[2, 3] = [5, -1]
        refused(c, blen, 3, 'earlier row')
        for v in (np.nan, -1e-9, np.inf):
            b = blen.copy(); b[2, 1, 1] = v
            refused(child, b, 1, '>= 0')
        with pytest.raises(_ffi.PhyloError) as e:
            ctx._check(ctx._lib.phylo_trees_loglik(ctx._h, 0, None, None, None, None, None, None))
        assert e.value.code == -1
        with pytest.raises(ValueError):
            ctx.trees_loglik(child[:, :3], blen[:, :3])


# ---- 7. the runner --------------------------------------------------------------------------------------------------------
def test_runner_score_trees():
    d = load_dataset('primate_data_wang')
    taxa, g = [str(t) for t in d['taxa']], d['genome']
    N = len(taxa)
    child, blen = random_trees(N, 12, 3)
    newicks = [TP.rows_to_newick(c, b, taxa) for c, b in zip(child, blen)]
    argv = ['--dataset', 'primate_data_wang', '--n_particles', '16', '--num_epoch', '1', '--batch_size', '512', '--jcmodel', 'true',
            '--seed', '2']
    for extra in ([], ['--tree_summary', 'true', '--tree_branches', 'true']):
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, 'trees.nwk')
            with open(path, 'w') as f:
                f.write('\n'.join(newicks) + '\n\n')
            p = subprocess.run([sys.executable, os.path.join(ROOT, 'runner.py')] + argv + ['--score_trees', path] + extra, cwd=tmp,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
            assert p.returncode == 0, p.stdout.decode()[-2000:]
            (res,) = glob.glob(os.path.join(tmp, 'results', '*', '*', '*', '*', 'tree_scores.json'))
            with open(res) as f:
                scores = json.load(f)
            mdl = scores['model']
            with make_ctx(g, np.array(mdl['Q']), jc=True, pi=np.array(mdl['pi'])) as ctx:
                ref = ctx.trees_loglik(child, blen)
                got = np.array([t['loglik'] for t in scores['trees']])
                assert got.shape == (3,) and np.isfinite(got).all()
                np.testing.assert_array_equal(bits(got), bits(ref))
                assert scores['best'] == int(np.argmax(ref))
                assert [t['newick'] for t in scores['trees']] == newicks
                if extra:
                    with open(os.path.join(os.path.dirname(res), 'map.tre')) as f:
                        c, b = TP.newick_to_rows(f.read(), taxa)
                    assert bits(scores['summary']['map']['loglik']) == bits(ctx.trees_loglik(c, b))[0]
                    assert np.isfinite(scores['summary']['consensus_bl']['loglik'])
                    tops = scores['summary']['topologies']
                    assert 1 <= len(tops) <= 10 and all(np.isfinite(t['loglik']) for t in tops)
                    assert bits(tops[0]['loglik']) == bits(scores['summary']['map']['loglik'])
                else:
                    assert 'summary' not in scores
