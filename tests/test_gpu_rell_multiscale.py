"""phylo_rell_multiscale on the device: the multiscale RELL bootstrap behind the AU test.  Counts, scores,
best and wins are replayed bit for bit against the library's host loop (phylo_debug_rell_multiscale_host) and, on the smallest
shapes, against tests/rell_ms_ref.py's rational arithmetic -- at the shapes where the epilogue's reduction can go wrong: tree
tiles with padded rows, ties across lanes and tiles, columns that are no multiple of 128, chunks that straddle scales, the
uint16 bound of a count, the panel edges --, through both instances of the product (scores stored and not); the anchor to
phylo_rell; refusals, company; end to end through runner.py --tree_tests_au.

Every test here needs Context.rell_multiscale: AttributeError without it."""
import functools
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import rell_ms_ref
import rell_ref
from phylo_amd import _ffi, model
from phylo_amd import treepost as TP
from phylo_amd import treetests as TT
from phylo_amd.datasets import load_dataset
from trees_cases import random_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SEED = 0x9E3779B97F4A7C15
S0, DRAWS, B0 = 37, (18, 37, 52), 150
K0 = len(DRAWS)
T_ALL = (1, 5, 64, 65, 130)
T_RAT, B_RAT = 5, 6                                     # the rational replay covers the corner up to 5 trees x 6 replicates per scale
hook = _ffi.debug_rell_multiscale_host


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host_of(f, draws, B, seed):
    return rell_ms_ref.host(f, draws, B, seed, hook)


@functools.lru_cache(maxsize=None)
def reference():
    """One reference for every T of T_ALL, computed once: a tree's chain is its own, so a call on the first T rows is the first T
    rows of the scores; best is recomputed per T from them."""
    f = rell_ref.factors(max(T_ALL), S0, 1037)
    ref = rell_ms_ref.host(f, DRAWS, B0, SEED, hook)
    x = _ffi.debug_rell_host(f, 0, 1, SEED)['site_loglik']
    ref.update(f=f, x=x, obs=rell_ref.observed(x[:T_RAT]))
    rat = np.stack([rell_ms_ref.rep_loglik(np.array([rell_ms_ref.counts(S0, DRAWS, k, b, SEED) for b in range(B_RAT)]), x[:T_RAT])
                    for k in range(K0)])
    np.testing.assert_array_equal(bits(ref['rep_loglik'][:, :T_RAT, :B_RAT]), bits(rat), err_msg="host loop against the rational replay")
    ref['rat'] = rat
    for a in ref.values():
        a.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def ctx():
    with _ffi.Context(4, 5, 10) as c:                    # the call reads no leaves: its S is its own
        yield c


def lex_best(R_KxTxB):
    return np.stack([rell_ref.first_argmax(R) for R in R_KxTxB])


def wins_of(best_KxB, T):
    return np.stack([np.bincount(b, minlength=T) for b in best_KxB]).astype(np.int64)


def check(ctx, f, draws, B, seed, want):
    """both instances of the product against `want` (counts [K][B][S], rep_loglik [K][T][B] of these T trees)"""
    T, S = f.shape
    K = len(draws)
    out = ctx.rell_multiscale(f, draws, B, seed, want_best=True, want_reps=True, want_counts=True)
    assert out['counts'].shape == (K, B, S) and out['rep_loglik'].shape == (K, T, B) and out['best'].shape == (K, B)
    assert out['wins'].shape == (K, T) and out['wins'].dtype == np.int64 and out['obs'].shape == (T,)
    np.testing.assert_array_equal(out['counts'], want['counts'], err_msg="counts")
    np.testing.assert_array_equal(out['counts'].sum(axis=2), np.repeat(np.array(draws)[:, None], B, axis=1))
    np.testing.assert_array_equal(bits(out['rep_loglik']), bits(want['rep_loglik']), err_msg="scores against the host loop")
    best = lex_best(out['rep_loglik'])                   # the first-max argmax of the fetched matrix
    np.testing.assert_array_equal(out['best'], best, err_msg="best, storing instance")
    assert out['best'].min() >= 0 and out['best'].max() < T                      # a padded row never wins
    np.testing.assert_array_equal(out['wins'], wins_of(best, T), err_msg="wins, storing instance")
    assert (out['wins'].sum(axis=1) == B).all()
    lean = ctx.rell_multiscale(f, draws, B, seed, want_best=True)                # the instance that stores no score
    assert sorted(lean) == ['best', 'obs', 'stats', 'wins']
    np.testing.assert_array_equal(lean['best'], out['best'], err_msg="best, non-storing instance")
    np.testing.assert_array_equal(lean['wins'], out['wins'], err_msg="wins, non-storing instance")
    np.testing.assert_array_equal(bits(lean['obs']), bits(out['obs']))
    np.testing.assert_array_equal(bits(out['obs']), bits(ctx.rell(f, 1, seed)['obs']), err_msg="obs is phylo_rell's")
    st = lean['stats']
    assert st['units'] == float(T) * S * K * B and st['sweep_ms'] > 0
    return out, lean


# ---- 1. tree tiles: one tile, a full tile, a tile of one real tree and 63 padded rows, three tiles -------------------------
@pytest.mark.parametrize("T", T_ALL)
def test_tree_tiles(ctx, T):
    ref = reference()
    want = {'counts': ref['counts'], 'rep_loglik': ref['rep_loglik'][:, :T]}
    out, lean = check(ctx, ref['f'][:T], DRAWS, B0, SEED, want)
    assert lean['stats']['n_launches'] == 5               # logs, counts, ones, product, join: one chunk
    if T >= 64:
        assert (ref['rep_loglik'][:, :T] < 0).all()       # every score is negative here: a padded row's +0.0 would win by value
    if T <= T_RAT:
        np.testing.assert_array_equal(bits(out['rep_loglik'][:, :, :B_RAT]), bits(ref['rat'][:, :T]), err_msg="scores against rationals")
        np.testing.assert_array_equal(bits(out['obs']), bits(ref['obs'][:T]), err_msg="observed scores against rationals")
        np.testing.assert_array_equal(out['best'][:, :B_RAT], np.stack([rell_ms_ref.best_lex(R) for R in ref['rat'][:, :T]]))


def test_factors_above_one(ctx):
    """every score positive: padded zeros lose by value too, and the reduction must not depend on the sign"""
    T = 65
    f = np.random.default_rng(8).uniform(1.1, 4.0, size=(T, S0))
    want = host_of(f, DRAWS, B0, SEED)
    assert (want['rep_loglik'] > 0).all()
    check(ctx, f, DRAWS, B0, SEED, want)


@pytest.mark.parametrize("T,lo,hi", [(130, 3, 70), (65, 3, 19)])
def test_ties(ctx, T, lo, hi):
    """two identical best rows: across tree tiles (3 and 70), and in one wave's tile on different lanes (3 and 19)"""
    f = rell_ref.factors(T, S0, 5, special=False).copy()                          # every factor below exp(-1) ...
    f[hi] = np.exp(np.random.default_rng(1).uniform(-0.5, -0.1, size=S0))         # ... this row above it at every site, and its copy
    f[lo] = f[hi]
    want = host_of(f, DRAWS, B0, SEED)
    out, lean = check(ctx, f, DRAWS, B0, SEED, want)
    np.testing.assert_array_equal(bits(out['rep_loglik'][:, lo]), bits(out['rep_loglik'][:, hi]))
    for o in (out, lean):
        assert (o['best'] == lo).all() and (o['wins'][:, lo] == B0).all() and (o['wins'][:, hi] == 0).all()
    np.testing.assert_array_equal(out['best'], want['best'])


# ---- 2. columns: 450 is no multiple of 128; chunks of 100 straddle the scales ------------------------------------------------
CHUNK_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import rell_ref
from phylo_amd import _ffi
f = rell_ref.factors(130, 37, 1037)[:65]
with _ffi.Context(4, 5, 10) as ctx:
    out = ctx.rell_multiscale(f, (18, 37, 52), 150, int(sys.argv[2]), want_best=True, want_reps=True, want_counts=True)
    lean = ctx.rell_multiscale(f, (18, 37, 52), 150, int(sys.argv[2]), want_best=True)
    np.savez(sys.argv[1], launches=out['stats']['n_launches'], lean_best=lean['best'], lean_wins=lean['wins'],
             **{k: v for k, v in out.items() if k != 'stats'})
"""


def test_chunks_that_straddle_scales_give_the_bits_of_one_chunk(ctx):
    """PHYLO_RELL_CHUNK is read when the context is created: a fresh process with 100 columns per chunk (scale edges at 150 and
    300 fall inside chunks), against this process's single chunk"""
    ref = reference()
    one = ctx.rell_multiscale(ref['f'][:65], DRAWS, B0, SEED, want_best=True, want_reps=True, want_counts=True)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'c100.npz')
        env = dict(os.environ, PHYLO_RELL_CHUNK='100')
        p = subprocess.run([sys.executable, '-c', CHUNK_SCRIPT % (ROOT, os.path.join(ROOT, 'tests')), path, str(SEED)], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        got = dict(np.load(path))
    assert int(got['launches']) == 2 + 3 * 5 and one['stats']['n_launches'] == 5          # 450 columns in 5 chunks
    for key in ('obs', 'rep_loglik'):
        np.testing.assert_array_equal(bits(got[key]), bits(one[key]), err_msg=key)
    for key in ('counts', 'best', 'wins'):
        np.testing.assert_array_equal(got[key], one[key], err_msg=key)
    np.testing.assert_array_equal(got['lean_best'], one['best'])
    np.testing.assert_array_equal(got['lean_wins'], one['wins'])
    np.testing.assert_array_equal(bits(one['rep_loglik']), bits(ref['rep_loglik'][:, :65]))


# ---- 3. count extremes and panel edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,draws", [(1, (1, 65535)), (33, (16, 33, 46)), (64, (32, 64, 90))])
def test_count_extremes_and_panel_edges(ctx, S, draws):
    """S = 1: a count of 65535, a full uint16; S = 33, 64: one site past a panel of 32, and two full panels"""
    T, B = 5, 20
    f = rell_ref.factors(T, S, 2000 + S)
    want = host_of(f, draws, B, SEED)
    out, _ = check(ctx, f, draws, B, SEED, want)
    if S == 1:
        assert (out['counts'][1] == 65535).all() and (out['counts'][0] == 1).all()
    x = _ffi.debug_rell_host(f, 0, 1, SEED)['site_loglik']
    rat = rell_ms_ref.rep_loglik(out['counts'][len(draws) - 1, :2], x)
    np.testing.assert_array_equal(bits(out['rep_loglik'][len(draws) - 1, :, :2]), bits(rat), err_msg="scores against rationals")


# ---- 4. the anchor: one scale of S draws is phylo_rell ------------------------------------------------------------------------
def test_one_scale_of_S_draws_is_phylo_rell(ctx):
    ref = reference()
    f = ref['f'][:65]
    plain = ctx.rell(f, B0, SEED, want_reps=True, want_counts=True)
    ms = ctx.rell_multiscale(f, (S0,), B0, SEED, want_best=True, want_reps=True, want_counts=True)
    np.testing.assert_array_equal(bits(ms['obs']), bits(plain['obs']))
    np.testing.assert_array_equal(ms['best'][0], plain['best'])
    np.testing.assert_array_equal(ms['wins'][0], plain['wins'])
    np.testing.assert_array_equal(ms['counts'][0], plain['counts'])
    np.testing.assert_array_equal(bits(ms['rep_loglik'][0]), bits(plain['rep_loglik']))
    lean = ctx.rell_multiscale(f, (S0,), B0, SEED, want_best=True)
    np.testing.assert_array_equal(lean['best'][0], plain['best'])
    np.testing.assert_array_equal(lean['wins'][0], plain['wins'])


# ---- 5. invariances ------------------------------------------------------------------------------------------------------------
def test_invariances(ctx):
    ref = reference()
    f = ref['f'][:65]
    kw = dict(want_best=True, want_reps=True, want_counts=True)
    a, b, c = ctx.rell_multiscale(f, DRAWS, B0, SEED, **kw), ctx.rell_multiscale(f, DRAWS, B0, SEED, **kw), ctx.rell_multiscale(f, DRAWS, B0, SEED + 1, **kw)
    for key in ('obs', 'rep_loglik'):
        np.testing.assert_array_equal(bits(a[key]), bits(b[key]), err_msg=key)
    for key in ('counts', 'best', 'wins'):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert not np.array_equal(a['counts'], c['counts'])
    np.testing.assert_array_equal(c['counts'][2, :3], np.array([rell_ms_ref.counts(S0, DRAWS, 2, r, SEED + 1) for r in range(3)]))
    np.testing.assert_array_equal(bits(a['obs']), bits(c['obs']))              # the observed scores know no seed
    # A scale does not depend on the company it rides in.  A call of K = 1 would put the scale at k = 0, another stream, so the
    # scale keeps its index and the scales before it become dummies that draw one site each (the choice among the two the
    # contract allows: a padded draws vector, not the hook).
    for k in range(K0):
        alone = ctx.rell_multiscale(f, (1,) * k + (DRAWS[k],), B0, SEED, **kw)
        np.testing.assert_array_equal(alone['counts'][k], a['counts'][k], err_msg="counts of scale %d alone" % k)
        np.testing.assert_array_equal(bits(alone['rep_loglik'][k]), bits(a['rep_loglik'][k]), err_msg="scores of scale %d alone" % k)
        np.testing.assert_array_equal(alone['best'][k], a['best'][k])
        np.testing.assert_array_equal(alone['wins'][k], a['wins'][k])
        if k:
            assert (alone['counts'][:k].sum(axis=2) == 1).all()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing(ctx):
    import ctypes as C
    T, B = 5, 20
    ref = reference()
    f = ref['f'][:T]
    want = {'counts': ref['counts'][:, :B], 'rep_loglik': ref['rep_loglik'][:, :T, :B]}

    def good():
        check(ctx, f, DRAWS, B, SEED, want)

    def refused(call, *what):
        with pytest.raises(_ffi.PhyloError) as e:
            call()
        assert e.value.code == -1, str(e.value)
        for x in what:
            assert x in str(e.value), str(e.value)
        good()                                             # a valid call on the same context is still correct

    good()
    for v in (0.0, -0.0, -2.0, np.inf, np.nan):
        g = f.copy()
        g[T - 1, S0 - 1] = v
        refused(lambda: ctx.rell_multiscale(g, DRAWS, B, SEED), 'tree %d, site %d' % (T - 1, S0 - 1))
    refused(lambda: ctx.rell_multiscale(f, DRAWS, 0, SEED), 'B=0')
    refused(lambda: ctx.rell_multiscale(f, DRAWS, (1 << 20) + 1, SEED), 'B=')
    refused(lambda: ctx.rell_multiscale(np.ones((1, 65536)), DRAWS, 1, SEED), 'S=65536')
    refused(lambda: ctx.rell_multiscale(f, (5,) * 65, B, SEED), 'K=65')
    refused(lambda: ctx.rell_multiscale(f, (18, 0, 52), B, SEED), 'k=1')
    refused(lambda: ctx.rell_multiscale(f, (18, 37, 65536), B, SEED), 'k=2', '65536')
    refused(lambda: ctx.rell_multiscale(f, (18, -3, 52), B, SEED), 'k=1')
    p = _ffi._ptr
    dr = np.array(DRAWS, dtype=np.int32)
    obs, wins = np.empty(T), np.empty((K0, T), dtype=np.int64)
    args = lambda T_, K_, d, o, w: (ctx._h, C.c_int(T_), C.c_int(S0), p(f), C.c_int(K_), d, C.c_int(B), C.c_uint64(SEED), o, w, None, None, None, None)
    refused(lambda: ctx._check(ctx._lib.phylo_rell_multiscale(*args(T, K0, None, p(obs), p(wins)))), 'NULL')
    refused(lambda: ctx._check(ctx._lib.phylo_rell_multiscale(*args(T, K0, p(dr), None, p(wins)))), 'NULL')
    refused(lambda: ctx._check(ctx._lib.phylo_rell_multiscale(*args(T, K0, p(dr), p(obs), None))), 'NULL')
    refused(lambda: ctx._check(ctx._lib.phylo_rell_multiscale(*args(0, K0, p(dr), p(obs), p(wins)))), 'T=0')
    refused(lambda: ctx._check(ctx._lib.phylo_rell_multiscale(*args(T, 0, p(dr), p(obs), p(wins)))), 'K=0')
    with pytest.raises(ValueError):
        ctx.rell_multiscale(f.reshape(-1), DRAWS, B, SEED)
    big = ctx.rell_multiscale(np.full((1, 65535), 0.5), (65535,), 1, SEED)    # the largest S and the largest draw count there are
    assert big['wins'].tolist() == [[1]]


# ---- 7. company -----------------------------------------------------------------------------------------------------------------
def test_the_sweep_a_pending_reverse_pass_a_summary_and_other_scratch_are_left_alone():
    g = load_dataset('primate_data')['genome'][:6, 100:170].copy()
    N, S, K, seed = 6, 70, 64, 5
    pi = np.array([[0.3, 0.2, 0.2, 0.3]])
    Q = model.get_Q(model.init_y_q())
    lam = np.linspace(5.0, 15.0, N - 1)
    ref = reference()
    f = ref['f'][:5]
    want = {'counts': ref['counts'][:, :20], 'rep_loglik': ref['rep_loglik'][:, :5, :20]}
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, pi, lam, lam[::-1].copy())
        out = ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        grad = ctx.sweep_backward()
        child, blen = TP.particle_trees(out['merges'], out['ancestors'], out['left_branches'], out['right_branches'], seed=seed)
        ll, sites = ctx.trees_loglik(child[:7], blen[:7], want_sites=True)
        plain = ctx.rell(sites, 40, SEED, want_reps=True)
        ctx.sweep_async(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)      # a bootstrap between a sweep and its pending reverse pass
        check(ctx, f, DRAWS, 20, SEED, want)                                   # (its own S: 37, not 70)
        grad2 = ctx.sweep_backward()
        again = ctx.sweep_fetch()
        for key in ('log_weights', 'log_likelihood', 'left_branches', 'right_branches'):
            np.testing.assert_array_equal(bits(again[key]), bits(out[key]), err_msg=key)
        np.testing.assert_array_equal(again['ancestors'], out['ancestors'])
        assert bits(again['logZ']) == bits(out['logZ'])
        for key in ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q'):
            np.testing.assert_array_equal(bits(grad2[key]), bits(grad[key]), err_msg=key)
        tab = ctx.tree_summary()                                               # ... and a tree summary keeps its branch pass
        own = ctx.rell_multiscale(sites, (35, 70, 98), 40, SEED, want_reps=True)
        np.testing.assert_array_equal(bits(own['rep_loglik']), bits(host_of(sites, (35, 70, 98), 40, SEED)['rep_loglik']))
        tb = ctx.tree_branches(tab)
        assert np.isfinite(tb['leaf_stats']).all()
        l2, s2 = ctx.trees_loglik(child[:7], blen[:7], want_sites=True)        # the tree-set scratch ...
        np.testing.assert_array_equal(bits(l2), bits(ll))
        np.testing.assert_array_equal(bits(s2), bits(sites))
        plain2 = ctx.rell(sites, 40, SEED, want_reps=True)                     # ... and the plain bootstrap's
        np.testing.assert_array_equal(bits(plain2['rep_loglik']), bits(plain['rep_loglik']))
        np.testing.assert_array_equal(plain2['wins'], plain['wins'])
        third = ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        np.testing.assert_array_equal(bits(third['log_weights']), bits(out['log_weights']))


# ---- 8. end to end --------------------------------------------------------------------------------------------------------------
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
OLD_KEYS = ['B', 'seed', 'best', 'obs', 'bp', 'p_kh', 'p_sh', 'c_elw']
NEW_KEYS = ['p_au', 'se_au', 'au_d', 'au_c', 'au_ok', 'au_scales', 'bp_scales']


def test_runner_tree_tests_au():
    d = load_dataset('primate_data_wang')
    taxa = [str(t) for t in d['taxa'][:6]]
    N, B, seed = len(taxa), 200, 3
    rng = np.random.default_rng(12)
    rows = [random_rows(N, rng) for _ in range(8)]
    newicks = [TP.rows_to_newick(c, b, taxa) for c, b in rows]
    argv = ['--dataset', 'primate_data_wang', '--n_particles', '16', '--num_epoch', '1', '--batch_size', '512', '--jcmodel', 'true',
            '--seed', '2']
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'trees.nwk')
        with open(path, 'w') as f:
            f.write('\n'.join(newicks) + '\n')
        for name, extra in (('au', ['--tree_tests_au', 'default']), ('plain', [])):
            cwd = os.path.join(tmp, name)
            os.makedirs(cwd)
            p = subprocess.run([sys.executable, '-c', RUNNER_SCRIPT % ROOT] + argv + ['--score_trees', path, '--tree_tests', '%d:%d' % (B, seed)]
                               + extra, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
            assert p.returncode == 0, p.stdout.decode()[-2000:]
            (res,) = glob.glob(os.path.join(cwd, 'results', '*', '*', '*', '*', 'tree_tests.json'))
            with open(res) as f:
                got[name] = json.load(f)
            with open(os.path.join(os.path.dirname(res), 'tree_scores.json')) as f:
                got[name + '_scores'] = json.load(f)
            with open(os.path.join(os.path.dirname(res), 'run_parameters.txt')) as f:
                assert ('tree_tests_au' in f.read()) == (name == 'au')
    au, plain = got['au'], got['plain']
    assert list(plain) == OLD_KEYS and list(au) == OLD_KEYS + NEW_KEYS
    for key in OLD_KEYS:
        assert au[key] == plain[key], key
    S = d['genome'].shape[1]
    sc = TT.au_scales(S, 'default')
    assert au['au_scales'] == {'r': sc['r'].tolist(), 'draws': sc['draws'].tolist(), 'sigma2': sc['sigma2'].tolist()}
    assert np.array(au['bp_scales']).shape == (10, 8) and len(au['p_au']) == 8
    # the same site factors once more: the model of tree_scores.json on the same slice, the trees as the runner read them
    m = got['au_scores']['model']
    rows = [TP.newick_to_rows(nw, taxa) for nw in newicks]
    child, blen = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    with _ffi.Context(16, N, S) as ctx:
        ctx.set_leaves(d['genome'][:6].copy())
        ctx.set_model(np.array(m['Q']), np.array(m['pi']).reshape(1, 4), np.full(N - 1, 10.0), np.full(N - 1, 10.0),
                      jc69_closed_form=m['jc69_closed_form'])
        ll, sites = ctx.trees_loglik(child, blen, want_sites=True)
        ms = ctx.rell_multiscale(sites, sc['draws'], B, seed)
    np.testing.assert_array_equal(bits(ms['obs']), bits(au['obs']), err_msg="the same site factors")
    np.testing.assert_array_equal(np.array(au['bp_scales']), ms['wins'] / float(B))
    fit = TT.au_test(ms['wins'], sc['sigma2'], B)
    assert au['p_au'] == fit['p_au'].tolist() and au['au_ok'] == [bool(x) for x in fit['au_ok']]
    for key, name in (('se_au', 'se_au'), ('au_d', 'd'), ('au_c', 'c')):
        assert [None if x != x else float(x) for x in fit[name]] == au[key], key
    assert all(0.0 <= v <= 1.0 for v in au['p_au'])
