"""phylo_rell on the device: the RELL bootstrap over the site factors of a scored tree set.  The contract
is replayed bit for bit -- counts, logs, replicate scores and observed scores against the library's host loop
(phylo_debug_rell_host) and against tests/rell_ref.py's rational arithmetic, every element --, at the shapes where a 16 x 16 x 4
tile, a 64-wide panel or a chunk edge can go wrong; best and wins by the tie rule; chunks, seeds, refusals, company; end to end
through trees_loglik, treetests and runner.py --tree_tests.

Every test here needs Context.rell: AttributeError without it."""
import functools
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import rell_ref
from phylo_amd import _ffi, model
from phylo_amd import treepost as TP
from phylo_amd.datasets import load_dataset, synthetic_alignment
from phylo_amd.treetests import tree_tests
from trees_cases import random_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SEED = 0x9E3779B97F4A7C15
T_ALL, B_ALL, S_ALL = (1, 15, 16, 17, 33), (1, 15, 16, 17, 40), (1, 3, 4, 5, 63, 64, 65, 130)
T_MAX, B_MAX = max(T_ALL), max(B_ALL)
T_RAT, B_RAT, S_RAT = 17, 17, 65                        # the rational replay covers the shapes up to 17 x 17 x 65


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def reference(S):
    """One reference per S, computed once: every (T, B) shape reads the first T rows and B replicates of it (a replicate's index is
    global and a tree's chain is its own, so a smaller call is a corner of the larger one)."""
    f = rell_ref.factors(T_MAX, S, 1000 + S)
    host = _ffi.debug_rell_host(f, 0, B_MAX, SEED)
    ref = {'f': f, 'counts': host['counts'], 'x': host['site_loglik'], 'rl': host['rep_loglik']}
    ref['obs'] = rell_ref.observed(ref['x'])            # (rational: the host hook has no such output)
    np.testing.assert_array_equal(ref['counts'], np.array([rell_ref.counts(S, b, SEED) for b in range(B_MAX)]))
    if S <= S_RAT:
        rat = rell_ref.rep_loglik(ref['counts'][:B_RAT], ref['x'][:T_RAT])
        np.testing.assert_array_equal(bits(ref['rl'][:T_RAT, :B_RAT]), bits(rat), err_msg="host loop against the rational replay")
        ref['rat'] = rat
    for a in ref.values():
        a.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def ctx():
    with _ffi.Context(4, 5, 10) as c:                    # the call reads no leaves: its S is its own
        yield c


def check(out, ref, T, B, S):
    assert out['counts'].shape == (B, S) and out['rep_loglik'].shape == (T, B) and out['site_loglik'].shape == (T, S)
    assert out['obs'].shape == (T,) and out['best'].shape == (B,) and out['wins'].shape == (T,)
    np.testing.assert_array_equal(out['counts'], ref['counts'][:B], err_msg="counts")
    assert (out['counts'].sum(axis=1) == S).all()
    np.testing.assert_array_equal(bits(out['site_loglik']), bits(ref['x'][:T]), err_msg="logs")
    np.testing.assert_array_equal(bits(out['rep_loglik']), bits(ref['rl'][:T, :B]), err_msg="replicate scores against the host loop")
    if 'rat' in ref and T <= T_RAT and B <= B_RAT:
        np.testing.assert_array_equal(bits(out['rep_loglik']), bits(ref['rat'][:T, :B]), err_msg="replicate scores against rationals")
    np.testing.assert_array_equal(bits(out['obs']), bits(ref['obs'][:T]), err_msg="observed scores")
    np.testing.assert_array_equal(out['best'], rell_ref.first_argmax(out['rep_loglik']), err_msg="best")
    np.testing.assert_array_equal(out['wins'], np.bincount(out['best'], minlength=T), err_msg="wins")
    assert int(out['wins'].sum()) == B


# ---- 1. the contract, every element, at the edges of tile, panel and workgroup ----------------------------------------------
@pytest.mark.parametrize("S", S_ALL)
def test_contract_bit_for_bit(ctx, S):
    ref = reference(S)
    np.testing.assert_array_equal(bits(ctx.math_probe(1, ref['f']).reshape(T_MAX, S)), bits(ref['x']), err_msg="the contract's log")
    assert np.isfinite(ref['x']).all() and ref['x'].min() < -700 and (ref['x'] == 0).any() and (ref['x'] > 0).any()
    for T in T_ALL:
        for B in B_ALL:
            out = ctx.rell(ref['f'][:T], B, SEED, want_reps=True, want_counts=True, want_logs=True)
            check(out, ref, T, B, S)
            st = out['stats']
            assert st['units'] == T * S * B and st['n_launches'] == 6 and st['sweep_ms'] > 0
    lean = ctx.rell(ref['f'], B_MAX, SEED)               # nothing optional asked for: the same required outputs
    assert sorted(lean) == ['best', 'obs', 'stats', 'wins']
    np.testing.assert_array_equal(bits(lean['obs']), bits(ref['obs']))
    np.testing.assert_array_equal(lean['best'], rell_ref.first_argmax(ref['rl']))


def test_more_than_one_workgroup_each_way(ctx):
    """65 trees and 130 replicates: two workgroups along either side, the second nearly empty; 37 sites: two panels"""
    T, B, S = 65, 130, 37
    f = rell_ref.factors(T, S, 77)
    host = _ffi.debug_rell_host(f, 0, B, SEED)
    out = ctx.rell(f, B, SEED, want_reps=True, want_counts=True, want_logs=True)
    ref = {'counts': host['counts'], 'x': host['site_loglik'], 'rl': host['rep_loglik'], 'obs': rell_ref.observed(host['site_loglik'])}
    check(out, ref, T, B, S)


def test_identical_rows_tie_to_the_lower_index(ctx):
    T, B, S = 17, 40, 65
    f = rell_ref.factors(T, S, 5).copy()
    f[11] = np.exp(np.random.default_rng(1).uniform(-1.5, -1.0, size=S))      # far above the others: it wins every replicate ...
    f[3] = f[11]                                                              # ... and so does its copy, at a lower index
    out = ctx.rell(f, B, SEED, want_reps=True)
    np.testing.assert_array_equal(bits(out['rep_loglik'][3]), bits(out['rep_loglik'][11]))
    assert (out['best'] == 3).all() and out['wins'][3] == B and out['wins'][11] == 0 and int(out['wins'].sum()) == B
    st = tree_tests(out['obs'], out['wins'], B, reps=out['rep_loglik'])
    assert st['best'] == 3 and st['p_kh'][11] == 1.0 and st['p_sh'][11] == 1.0 and st['bp'][11] == 0.0


def test_seeds(ctx):
    ref = reference(65)
    a = ctx.rell(ref['f'][:17], 40, SEED, want_reps=True, want_counts=True)
    b = ctx.rell(ref['f'][:17], 40, SEED, want_reps=True, want_counts=True)
    c = ctx.rell(ref['f'][:17], 40, SEED + 1, want_reps=True, want_counts=True)
    for key in ('obs', 'rep_loglik'):
        np.testing.assert_array_equal(bits(a[key]), bits(b[key]), err_msg=key)
    for key in ('counts', 'best', 'wins'):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert not np.array_equal(a['counts'], c['counts'])
    np.testing.assert_array_equal(c['counts'], np.array([rell_ref.counts(65, r, SEED + 1) for r in range(40)]))
    np.testing.assert_array_equal(bits(a['obs']), bits(c['obs']))            # the observed scores know no seed


# ---- 2. chunks ----------------------------------------------------------------------------------------------------------------
CHUNK_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import rell_ref
from phylo_amd import _ffi
f = rell_ref.factors(17, 65, 1065)
with _ffi.Context(4, 5, 10) as ctx:
    out = ctx.rell(f, 40, int(sys.argv[2]), want_reps=True, want_counts=True, want_logs=True)
    np.savez(sys.argv[1], launches=out['stats']['n_launches'], **{k: v for k, v in out.items() if k != 'stats'})
"""


def test_chunks_give_the_bits_of_one_chunk():
    """PHYLO_RELL_CHUNK is read when the context is created: a fresh process per setting"""
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for chunk in ('0', '7', '16'):
            out = os.path.join(tmp, 'c%s.npz' % chunk)
            env = dict(os.environ, PHYLO_RELL_CHUNK=chunk)
            p = subprocess.run([sys.executable, '-c', CHUNK_SCRIPT % (ROOT, os.path.join(ROOT, 'tests')), out, str(SEED)], env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
            assert p.returncode == 0, p.stdout.decode()[-2000:]
            got[chunk] = dict(np.load(out))
    assert [int(got[c]['launches']) for c in ('0', '7', '16')] == [6, 3 + 3 * 6, 3 + 3 * 3]     # 40 replicates in 1, 6 and 3 chunks
    for chunk in ('7', '16'):
        for key in ('obs', 'rep_loglik', 'site_loglik'):
            np.testing.assert_array_equal(bits(got[chunk][key]), bits(got['0'][key]), err_msg="%s at chunk %s" % (key, chunk))
        for key in ('counts', 'best', 'wins'):
            np.testing.assert_array_equal(got[chunk][key], got['0'][key], err_msg="%s at chunk %s" % (key, chunk))
    host = _ffi.debug_rell_host(rell_ref.factors(17, 65, 1065), 0, 40, SEED)
    np.testing.assert_array_equal(bits(got['0']['rep_loglik']), bits(host['rep_loglik']))
    np.testing.assert_array_equal(got['0']['counts'], host['counts'])


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing(ctx):
    T, B, S = 17, 17, 65
    ref = reference(S)
    f = ref['f'][:T]

    def good():
        out = ctx.rell(f, B, SEED, want_reps=True, want_counts=True, want_logs=True)
        check(out, ref, T, B, S)

    def refused(call, *what):
        with pytest.raises(_ffi.PhyloError) as e:
            call()
        assert e.value.code == -1, str(e.value)
        for x in what:
            assert x in str(e.value), str(e.value)
        good()                                             # a valid call on the same context is still correct

    good()
    for v in (0.0, -0.0, -1e-300, -2.0, np.inf, -np.inf, np.nan):
        g = f.copy()
        g[T - 1, S - 1] = v
        refused(lambda: ctx.rell(g, B, SEED), 'tree %d, site %d' % (T - 1, S - 1))
    refused(lambda: ctx.rell(f, 0, SEED), 'B=0')
    refused(lambda: ctx.rell(f, (1 << 20) + 1, SEED), 'B=')
    refused(lambda: ctx.rell(np.ones((1, 65536)), 1, SEED), 'S=65536')
    obs, best, wins = np.empty(T), np.empty(B, dtype=np.int32), np.empty(T, dtype=np.int64)
    p = _ffi._ptr
    import ctypes as C
    args = lambda o, b, w: (ctx._h, C.c_int(T), C.c_int(S), p(f), C.c_int(B), C.c_uint64(SEED), o, b, w, None, None, None, None)
    refused(lambda: ctx._check(ctx._lib.phylo_rell(*args(None, p(best), p(wins)))), 'NULL')
    refused(lambda: ctx._check(ctx._lib.phylo_rell(*args(p(obs), None, p(wins)))), 'NULL')
    refused(lambda: ctx._check(ctx._lib.phylo_rell(*args(p(obs), p(best), None))), 'NULL')
    refused(lambda: ctx._check(ctx._lib.phylo_rell(ctx._h, C.c_int(0), C.c_int(S), p(f), C.c_int(B), C.c_uint64(SEED), p(obs), p(best),
                                                   p(wins), None, None, None, None)), 'T=0')
    with pytest.raises(ValueError):
        ctx.rell(f.reshape(-1), B, SEED)
    assert ctx.rell(np.full((1, 65535), 0.5), 1, SEED)['wins'].tolist() == [1]        # the largest S there is


# ---- 4. company ---------------------------------------------------------------------------------------------------------------
def test_the_sweep_a_pending_reverse_pass_and_a_summary_are_left_alone():
    g = load_dataset('primate_data')['genome'][:6, 100:170].copy()
    N, S, K, seed = 6, 70, 64, 5
    pi = np.array([[0.3, 0.2, 0.2, 0.3]])
    Q = model.get_Q(model.init_y_q())
    lam = np.linspace(5.0, 15.0, N - 1)
    ref = reference(65)
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, pi, lam, lam[::-1].copy())
        out = ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        grad = ctx.sweep_backward()
        child, blen = TP.particle_trees(out['merges'], out['ancestors'], out['left_branches'], out['right_branches'], seed=seed)
        ll, sites = ctx.trees_loglik(child[:7], blen[:7], want_sites=True)
        ctx.sweep_async(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)      # a bootstrap between a sweep and its pending reverse pass
        boot = ctx.rell(ref['f'][:17], 17, SEED, want_reps=True, want_counts=True, want_logs=True)      # (its own S: 65, not 70)
        check(boot, ref, 17, 17, 65)
        grad2 = ctx.sweep_backward()
        again = ctx.sweep_fetch()
        for key in ('log_weights', 'log_likelihood', 'left_branches', 'right_branches'):
            np.testing.assert_array_equal(bits(again[key]), bits(out[key]), err_msg=key)
        np.testing.assert_array_equal(again['ancestors'], out['ancestors'])
        assert bits(again['logZ']) == bits(out['logZ'])
        for key in ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q'):
            np.testing.assert_array_equal(bits(grad2[key]), bits(grad[key]), err_msg=key)
        tab = ctx.tree_summary()                                               # ... and a tree summary keeps its branch pass
        own = ctx.rell(sites, 40, SEED, want_reps=True)
        np.testing.assert_array_equal(bits(own['rep_loglik']), bits(_ffi.debug_rell_host(sites, 0, 40, SEED)['rep_loglik']))
        tb = ctx.tree_branches(tab)
        assert np.isfinite(tb['leaf_stats']).all()
        l2, s2 = ctx.trees_loglik(child[:7], blen[:7], want_sites=True)        # the tree-set scratch too
        np.testing.assert_array_equal(bits(l2), bits(ll))
        np.testing.assert_array_equal(bits(s2), bits(sites))
        third = ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        np.testing.assert_array_equal(bits(third['log_weights']), bits(out['log_weights']))


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------
def some_trees(N, seed, n):
    rng = np.random.default_rng(seed)
    rows = [random_rows(N, rng) for _ in range(n)]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])


def test_scores_to_statistics():
    N, S, n, B = 6, 130, 8, 200
    g = synthetic_alignment(N, S, seed=12)['genome'].copy()
    child, blen = some_trees(N, 3, n)
    with _ffi.Context(4, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(model.get_Q(model.init_y_q()), np.full(4, 0.25), np.full(N - 1, 10.0), np.full(N - 1, 10.0))
        ll, sites = ctx.trees_loglik(child, blen, want_sites=True)
        out = ctx.rell(sites, B, 3, want_reps=True)
    host = _ffi.debug_rell_host(sites, 0, B, 3)
    np.testing.assert_array_equal(bits(out['rep_loglik']), bits(host['rep_loglik']))
    obs = rell_ref.observed(host['site_loglik'])
    np.testing.assert_array_equal(bits(out['obs']), bits(obs))
    # the chain and the site-product form of the scoring call agree to the last bits, not bit for bit: S - 1
    # roundings of sums of one sign in the chain, an ulp in every log, less in the product form -- within (S + 4) 2^-53, relative
    np.testing.assert_allclose(out['obs'], ll, rtol=(S + 4) * 2.0 ** -53, atol=0)
    got = tree_tests(out['obs'], out['wins'], B, reps=out['rep_loglik'])
    want = rell_ref.tree_tests_loops(obs.tolist(), host['rep_loglik'].tolist())
    for key in ('bp', 'p_kh', 'p_sh', 'c_elw'):
        np.testing.assert_allclose(got[key], want[key], rtol=0, atol=1e-12, err_msg=key)
    assert got['bp'].sum() == pytest.approx(1.0, abs=1e-12) and got['p_kh'][got['best']] == 1.0


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


def test_runner_tree_tests():
    d = load_dataset('primate_data_wang')
    taxa = [str(t) for t in d['taxa'][:6]]
    N = len(taxa)
    child, blen = some_trees(N, 12, 8)
    newicks = [TP.rows_to_newick(c, b, taxa) for c, b in zip(child, blen)]
    argv = ['--dataset', 'primate_data_wang', '--n_particles', '16', '--num_epoch', '1', '--batch_size', '512', '--jcmodel', 'true',
            '--seed', '2']
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'trees.nwk')
        with open(path, 'w') as f:
            f.write('\n'.join(newicks) + '\n')
        p = subprocess.run([sys.executable, '-c', RUNNER_SCRIPT % ROOT] + argv + ['--score_trees', path, '--tree_tests', '200:3'], cwd=tmp,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        (res,) = glob.glob(os.path.join(tmp, 'results', '*', '*', '*', '*', 'tree_tests.json'))
        with open(res) as f:
            tt = json.load(f)
        with open(os.path.join(os.path.dirname(res), 'tree_scores.json')) as f:
            scores = json.load(f)
        with open(os.path.join(os.path.dirname(res), 'run_parameters.txt')) as f:
            assert 'tree_tests : 200:3' in f.read()
    assert tt['B'] == 200 and tt['seed'] == 3 and list(scores) == ['model', 'trees', 'best']
    for key in ('obs', 'bp', 'p_kh', 'p_sh', 'c_elw'):
        assert len(tt[key]) == 8 and np.isfinite(tt[key]).all(), key
    assert sum(tt['bp']) == pytest.approx(1.0, abs=1e-12) and sum(tt['c_elw']) == pytest.approx(1.0, abs=1e-12)
    assert tt['best'] == int(np.argmax(tt['obs'])) == scores['best'] and tt['p_kh'][tt['best']] == 1.0 and tt['p_sh'][tt['best']] == 1.0
    S = d['genome'].shape[1]
    np.testing.assert_allclose(tt['obs'], [t['loglik'] for t in scores['trees']], rtol=(S + 4) * 2.0 ** -53, atol=0)   # (as above)
