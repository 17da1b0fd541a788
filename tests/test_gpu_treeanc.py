"""phylo_trees_ancestral on the device: the marginal posterior of every state at every internal node and
site of a set of trees, the most probable state and its posterior.  loglik is held to phylo_trees_loglik's bits; post to the NumPy
restatement (treeanc_ref.py, fed with the device's own branch matrices) within TOL_ANC |value|, TOL_ANC = 8 E_REF_ANC 2^-53 with
E_REF_ANC the restatement's own error against 50-digit arithmetic (treeanc_cases.py) -- a bound set before the kernel ran; state
and pmax to the device's own post bit for bit.  Then: the same bits every way, a workgroup that takes several items, 129 and 512
taxa, the per-site NaN rule, what the call leaves alone, refusals, reuse, runner.py --score_ancestral.

Every test here needs Context.trees_ancestral: AttributeError without it."""
import ctypes as C
import glob
import itertools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import treeanc_cases as AC
import treeanc_ref as AR
import trees_edges_cases as EC
from phylo_amd import _ffi, model
from phylo_amd import ancestral as A
from phylo_amd import treepost as TP
from phylo_amd.datasets import load_dataset
from test_gpu_trees_edges import compute_units
from test_gpu_trees_loglik import CASES, PI, alignment, bits, gtr_Q, make_ctx, random_trees
from treeanc_cases import PRIOR, T, TOL_ANC

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ALL = dict(want_post=True, want_state=True, want_pmax=True)


def device_matrices(ctx, blen):
    """the device's own branch matrices (ctx.expm_batched): expm differences stay out of the comparison"""
    return ctx.expm_batched(np.asarray(blen).reshape(-1)).reshape(np.shape(blen) + (4, 4))


def own_argmax(post, state, pmax, what):
    """state is the argmax of the device's own post (the lowest index among equals, NOSTATE where any is NaN) and pmax those bits"""
    st, pm = AR.map_states(post)
    np.testing.assert_array_equal(state, st, err_msg=what + ": state against the device's own post")
    np.testing.assert_array_equal(bits(pmax), bits(pm), err_msg=what + ": pmax against the device's own post")
    assert state.dtype == np.uint8


def against_reference(what, ctx, child, blen, g, got):
    """post within TOL_ANC of the restatement, state equal to the restatement's wherever that is decided; returns the restatement"""
    ll, post, state, pmax = got
    rll, rpost, rstate, rpmax, L = AR.trees_ancestral(child, device_matrices(ctx, blen), PRIOR, g)
    assert np.isfinite(rpost).all() and (L >= AR.FLOOR).all()
    np.testing.assert_allclose(ll, rll, rtol=1e-12, atol=0)
    ok, worst = AC.within_tol(post, rpost)
    same = float((bits(post) == bits(rpost)).mean())
    sums = float(np.abs(post.sum(axis=-1) - 1.0).max())
    print("%s: worst |device - reference| = %.3g of the bound (TOL_ANC %.3g); %.2f %% of post bit-identical; worst |sum - 1| = %.3g"
          % (what, worst, TOL_ANC, 100 * same, sums))
    assert np.isfinite(post).all() and ok.all(), (what, worst)
    own_argmax(post, state, pmax, what)
    dec = AC.decided(rpost)
    share = 1.0 - float(dec.mean())
    assert share < AC.MAX_EXCLUDED, (what, share)
    np.testing.assert_array_equal(state[dec], rstate[dec], err_msg=what + ": state against the restatement")
    return rll, rpost, rstate, rpmax


def same_bits(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        if a.dtype == np.uint8:
            np.testing.assert_array_equal(a, b, err_msg="%s: output %d" % (what, k))
        else:
            np.testing.assert_array_equal(bits(a), bits(b), err_msg="%s: output %d" % (what, k))


# ---- 1. the cases of section 11, several chunks each ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_reference(name, monkeypatch):
    g, Q, child, blen, jc, n, tile = AC.case_inputs(name)
    N, S = g.shape[0], g.shape[1]
    if N > 2:
        assert (blen == 0).any()                                          # trees with zero-length branches
    chunk = 2 if n < T else 5
    monkeypatch.setenv('PHYLO_TREES_CHUNK', str(chunk))                   # read when the context is created: several chunks
    with make_ctx(g, Q, jc=jc, tile=tile) as ctx:
        got = ctx.trees_ancestral(child, blen, prior=PRIOR, **ALL)
        st = ctx.last_trees_stats
        assert got[1].shape == (n, N - 1, S, 4) and got[2].shape == (n, N - 1, S) and got[3].shape == (n, N - 1, S)
        assert st['units'] == n * S * (N - 1) and st['sweep_ms'] > 0
        per_chunk = 3 if CASES[name].get('generic') else 4                # coded leaves: the gap rows of M too
        assert st['n_launches'] == -(-n // chunk) * per_chunk
        np.testing.assert_array_equal(bits(got[0]), bits(ctx.trees_loglik(child, blen, prior=PRIOR)), err_msg="loglik against phylo_trees_loglik")
        assert np.isfinite(got[0]).all()
        against_reference(name, ctx, child, blen, g, got)
        rev = ctx.trees_ancestral(child[::-1], blen[::-1], prior=PRIOR, **ALL)      # a tree's bits do not depend on its place
        same_bits([a[::-1] for a in rev], got, "the trees in reverse order")


def test_prior_none_is_the_models_pi():
    g = alignment(7, 70, 3, gaps=True)
    pi = np.array([0.4, 0.3, 0.2, 0.1])
    child, blen = random_trees(7, 9, 5)
    with make_ctx(g, gtr_Q(), pi=pi) as ctx:
        a, b = ctx.trees_ancestral(child, blen), ctx.trees_ancestral(child, blen, prior=pi)
        assert len(a) == 3                                               # the default: loglik, post, state
        same_bits(a, b, "prior None against the model's pi")
        assert not np.array_equal(a[1], ctx.trees_ancestral(child, blen, prior=PI)[1])
        with pytest.raises(ValueError):
            ctx.trees_ancestral(child, blen, want_post=False, want_state=False)


# ---- 2. the same bits every way ---------------------------------------------------------------------------------------------
def test_same_bits_every_way(monkeypatch):
    g = alignment(12, 130, 31, gaps=True)
    child, blen = random_trees(12, 6)
    got = {}
    for chunk in ('0', '5', '1'):
        monkeypatch.setenv('PHYLO_TREES_CHUNK', chunk)
        with make_ctx(g, gtr_Q(), tile=64) as ctx:
            got[chunk] = ctx.trees_ancestral(child, blen, **ALL)
            assert ctx.last_trees_stats['n_launches'] == 4 * {'0': 1, '5': 8, '1': 37}[chunk]
            same_bits(ctx.trees_ancestral(child, blen, **ALL), got[chunk], "a second call")
            if chunk == '5':
                rev = ctx.trees_ancestral(child[::-1], blen[::-1], **ALL)
                same_bits([a[::-1] for a in rev], got[chunk], "the set reversed")
                for flags in itertools.product((False, True), repeat=3):  # which outputs are asked for changes no bit
                    if not any(flags):
                        continue
                    part = ctx.trees_ancestral(child, blen, want_post=flags[0], want_state=flags[1], want_pmax=flags[2])
                    want = [got[chunk][0]] + [got[chunk][1 + k] for k in range(3) if flags[k]]
                    same_bits(part, want, "outputs %r" % (flags,))
    for chunk in ('5', '1'):
        same_bits(got[chunk], got['0'], "chunks of " + chunk)


# ---- 3. more items than workgroups ------------------------------------------------------------------------------------------
def test_strided_items(monkeypatch):
    """N = 5, S = 192 in tiles of 64 (three tiles), T trees with 3 T = 8 CUs + 5 items (or the next multiple of three above):
    every workgroup of the capped grid takes a second item of another tree over the same node store, against the same trees in
    chunks of one item per workgroup"""
    cus = compute_units()
    cap = EC.updown_cap(5, cus)
    assert cap == 8 * cus
    n = -(-(cap + 5) // 3)
    g = alignment(5, 192, 77, gaps=True)
    child, blen = random_trees(5, 78, n)
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, gtr_Q(), pi=PRIOR, tile=64) as ctx:
        assert -(-192 // ctx.site_tile()) == 3 and 3 * n > cap and (3 * n) % cap != 0
        full = ctx.trees_ancestral(child, blen, **ALL)
        assert ctx.last_trees_stats['n_launches'] == 4                   # one chunk: items > grid, workgroups stride
        np.testing.assert_array_equal(bits(full[0]), bits(ctx.trees_loglik(child, blen)))
        sample = sorted(set(range(4)) | set(range(cap // 3 - 2, n)))      # the first trees, and every tree of a second item
        against_reference("strided", ctx, child[sample], blen[sample], g, [a[sample] for a in full])
    chunk = cap // 3
    monkeypatch.setenv('PHYLO_TREES_CHUNK', str(chunk))
    with make_ctx(g, gtr_Q(), pi=PRIOR, tile=64) as ctx:
        parts = ctx.trees_ancestral(child, blen, **ALL)
        assert ctx.last_trees_stats['n_launches'] == -(-n // chunk) * 4
    same_bits(full, parts, "strided against one item per workgroup")


# ---- 4. 512 and 129 taxa ----------------------------------------------------------------------------------------------------
def many_taxa_tree(N):
    """one balanced tree of N taxa (trees_edges_cases' generating tree and lengths) and S = 130 sites simulated along it"""
    from treegrad_cases import simulate
    name = 'balanced-N%d' % N
    _, child, blen, Q = EC.big_case(name)
    c0, b0 = EC.SHAPES['balanced'](N, np.random.default_rng(EC.SEEDS.get(name, 12)))
    assert c0.tobytes() == child[0].tobytes()
    g = simulate(c0, b0 + 0.05, Q, PRIOR, 130, np.random.default_rng(130 + N))
    return g, child[:1], blen[:1], Q


@pytest.mark.parametrize("N", [512, 129])
def test_many_taxa(N, monkeypatch):
    g, child, blen, Q = many_taxa_tree(N)
    depth = _ffi.debug_tree_schedule(child[0], blen[0])[1]
    assert depth == {512: 9, 129: 7}[N]                                   # 9 slots: the deepest stack 512 taxa can need
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:                        # three tiles, the last with 2 live lanes
        got = ctx.trees_ancestral(child, blen, **ALL)
        assert ctx.last_trees_stats['n_launches'] == 4 and ctx.last_trees_stats['units'] == 130 * (N - 1)
        np.testing.assert_array_equal(bits(got[0]), bits(ctx.trees_loglik(child, blen)))
        against_reference("balanced-N%d" % N, ctx, child, blen, g, got)


# ---- 5. the NaN rule, per site ----------------------------------------------------------------------------------------------
def test_nan_rule_is_per_site():
    g, child, blen, Q = EC.scaled_base()
    S = g.shape[1]
    with make_ctx(g, Q, pi=PRIOR, tile=64) as ctx:
        base = ctx.trees_ancestral(child, blen, **ALL)
        L0 = AR.trees_ancestral(child, device_matrices(ctx, blen), PRIOR, g)[4]
    assert np.isfinite(base[1]).all() and (L0 > 2.0 ** -200).all()
    e = EC.scaled_exponents('just-below', L0)
    for k, s in enumerate(EC.SCALED_SITES):                               # ONE site just below the floor: each of the four in turn
        only = np.where(np.arange(len(e)) == k, e, 0)
        gs = EC.scaled_leaves(g, only)
        others = [x for x in range(S) if x != s]
        with make_ctx(gs, Q, pi=PRIOR, tile=64) as ctx:
            ll, post, state, pmax = ctx.trees_ancestral(child, blen, **ALL)
            scored, sites = ctx.trees_loglik(child, blen, want_sites=True)
        assert (sites[:, s] < AR.FLOOR).all() and (sites[:, s] > 0).all() and (sites[:, others] >= 2.0 ** -200).all()
        np.testing.assert_array_equal(bits(ll), bits(scored), err_msg="loglik stays the scoring call's")
        assert np.isfinite(ll).all()
        assert np.isnan(post[:, :, s]).all() and (state[:, :, s] == _ffi.ANC_NOSTATE).all() and np.isnan(pmax[:, :, s]).all()
        same_bits([post[:, :, others], state[:, :, others], pmax[:, :, others]], [a[:, :, others] for a in base[1:]],
                  "site %d below the floor: every other column" % s)


def test_nan_rule_generic_zero_row():
    N, S = 5, 70
    g = alignment(N, S, 22, generic=True)
    child, blen = random_trees(N, 4, 3)
    with make_ctx(g, gtr_Q()) as ctx:
        base = ctx.trees_ancestral(child, blen, prior=PI, **ALL)
    g2 = g.copy()
    g2[2, 66] = 0.0                                                       # a generic leaf row of zeros kills the site in every tree
    others = [x for x in range(S) if x != 66]
    with make_ctx(g2, gtr_Q()) as ctx:
        ll, post, state, pmax = ctx.trees_ancestral(child, blen, prior=PI, **ALL)
        np.testing.assert_array_equal(bits(ll), bits(ctx.trees_loglik(child, blen, prior=PI)))
    assert (ll == -np.inf).all()
    assert np.isnan(post[:, :, 66]).all() and (state[:, :, 66] == 255).all() and np.isnan(pmax[:, :, 66]).all()
    same_bits([post[:, :, others], state[:, :, others], pmax[:, :, others]], [a[:, :, others] for a in base[1:]], "every other column")


# ---- 6. what the call leaves alone ------------------------------------------------------------------------------------------
def test_sweep_backward_summary_and_scratch_are_left_alone():
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
        ctx.sweep_async(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        child, blen = TP.particle_trees(out['merges'], out['ancestors'], out['left_branches'], out['right_branches'], seed=seed)
        ll, sites = ctx.trees_loglik(child[:7], blen[:7], want_sites=True)
        rl = ctx.rell(sites, 50, 3, want_reps=True)
        tg = ctx.trees_grad(child, blen, want_curv=True)
        nni = ctx.trees_nni(child[:7], blen[:7])
        anc = ctx.trees_ancestral(child, blen, **ALL)                      # between a sweep and its pending reverse pass
        assert np.isfinite(anc[1]).all() and (anc[2] < 4).all()
        np.testing.assert_array_equal(bits(anc[0][:7]), bits(ll))
        grad2 = ctx.sweep_backward()
        again = ctx.sweep_fetch()
        for key in ('log_weights', 'log_likelihood', 'left_branches', 'right_branches'):
            np.testing.assert_array_equal(bits(again[key]), bits(out[key]), err_msg=key)
        np.testing.assert_array_equal(again['ancestors'], out['ancestors'])
        assert bits(again['logZ']) == bits(out['logZ'])
        for key in ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q'):
            np.testing.assert_array_equal(bits(grad2[key]), bits(grad[key]), err_msg=key)
        # the scratch of sections 11 to 14: the same calls give the same bits afterwards
        l2, s2 = ctx.trees_loglik(child[:7], blen[:7], want_sites=True)
        np.testing.assert_array_equal(bits(s2), bits(sites))
        np.testing.assert_array_equal(bits(ctx.rell(sites, 50, 3, want_reps=True)['rep_loglik']), bits(rl['rep_loglik']))
        same_bits(ctx.trees_grad(child, blen, want_curv=True), tg, "trees_grad afterwards")
        same_bits(ctx.trees_nni(child[:7], blen[:7]), nni, "trees_nni afterwards")
        # a tree summary made before the call still has its branch pass
        tab = ctx.tree_summary()
        ctx.trees_ancestral(child[:3], blen[:3])
        tb = ctx.tree_branches(tab)
        assert np.isfinite(tb['leaf_stats']).all()
        third = ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)   # the next sweep's bits
        np.testing.assert_array_equal(bits(third['log_weights']), bits(out['log_weights']))


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing():
    N, S = 5, 70
    g = alignment(N, S, 41)
    child, blen = random_trees(N, 8, 4)
    child[2] = np.array([[0, 1], [2, 3], [6, 4], [5, 7]], dtype=np.int32)
    with _ffi.Context(4, N, S) as ctx:
        with pytest.raises(_ffi.PhyloError) as e:
            ctx.trees_ancestral(child, blen)
        assert e.value.code == -6
        ctx.set_leaves(g)
        ctx.set_model(gtr_Q(), PI, np.full(N - 1, 10.0), np.full(N - 1, 10.0))
        ref = ctx.trees_ancestral(child, blen, **ALL)

        def refused(call, what):
            with pytest.raises(_ffi.PhyloError) as e:
                call()
            assert e.value.code == -1 and what in str(e.value), str(e.value)
            same_bits(ctx.trees_ancestral(child, blen, **ALL), ref, "a valid call after a refusal")

        c = child.copy(); c[2, 2] = [6, 0]
        refused(lambda: ctx.trees_ancestral(c, blen), 'tree 2, row 2')        # a leaf used twice
        c2 = child.copy(); c2[2, 3] = [5, -1]
        refused(lambda: ctx.trees_ancestral(c2, blen), 'tree 2, row 3')       # no child at all
        for v in (np.nan, -1e-9, np.inf):
            b = blen.copy(); b[2, 1, 1] = v
            refused(lambda: ctx.trees_ancestral(child, b), 'tree 2, row 1')   # a negative (or non-finite) length
        ch, bl = np.ascontiguousarray(child, dtype=np.int32), np.ascontiguousarray(blen)
        ll, st = np.empty(4), np.empty((4, N - 1, S), dtype=np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        raw = lambda *a: ctx._check(ctx._lib.phylo_trees_ancestral(ctx._h, C.c_int(4), p(ch), p(bl), None, *a))
        refused(lambda: raw(p(ll), None, None, None, None), 'all three')      # all three outputs NULL
        refused(lambda: raw(None, None, p(st), None, None), 'NULL')           # NULL loglik
        refused(lambda: ctx._check(ctx._lib.phylo_trees_ancestral(ctx._h, C.c_int(4), None, p(bl), None, p(ll), None, p(st), None, None)), 'NULL')
        with pytest.raises(ValueError):
            ctx.trees_ancestral(child[:, :3], blen[:, :3])


# ---- 8. reuse ---------------------------------------------------------------------------------------------------------------
def device_bytes_free():
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert _ffi.load().hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_reuse_keeps_device_memory_flat(monkeypatch):
    """contexts created, called and destroyed again and again, and one long-lived context called again and again: a leak of the
    call's slab (here 24 MB of staged outputs and the node stores) grows linearly -- by 10 slabs over each half of the run -- and
    device memory that is flat does not.  Memory another process takes on the same device would have to arrive in both halves."""
    N, S, n = 12, 2050, 32
    g = alignment(N, S, 9, gaps=True)
    child, blen = random_trees(N, 3, n)
    slab = n * (N - 1) * S * 33
    monkeypatch.delenv('PHYLO_TREES_CHUNK', raising=False)
    first = None

    def cycle():
        nonlocal first
        with make_ctx(g, gtr_Q()) as ctx:
            got = ctx.trees_ancestral(child, blen)
        if first is None:
            first = got
        same_bits(got, first, "a fresh context")

    marks = []
    for rep in range(3):
        for _ in range(10 if rep else 2):                                 # two cycles to warm up, then two halves of ten
            cycle()
        marks.append(device_bytes_free())
    grown = [marks[0] - marks[1], marks[1] - marks[2]]
    print("free device memory after 2 / 12 / 22 contexts: %r (slab %d bytes)" % (marks, slab))
    assert min(grown) < slab, grown
    with make_ctx(g, gtr_Q()) as ctx:
        ctx.trees_ancestral(child, blen)
        marks = [device_bytes_free()]
        for rep in range(2):
            for _ in range(10):
                same_bits(ctx.trees_ancestral(child, blen), first, "a long-lived context")
            marks.append(device_bytes_free())
        grown = [marks[0] - marks[1], marks[1] - marks[2]]
        print("free device memory of one context after 1 / 11 / 21 calls: %r" % (marks,))
        assert min(grown) < slab, grown


# ---- 9. the runner ----------------------------------------------------------------------------------------------------------
def test_runner_score_ancestral():
    d = load_dataset('primate_data_wang')                               # primates_small.fa: N = 9, S = 738
    taxa = [str(t) for t in d['taxa']]
    g = d['genome']
    N, S = g.shape[0], g.shape[1]
    child, blen = random_trees(N, 12, 3)
    blen = blen + 0.02
    newicks = [TP.rows_to_newick(c, b, taxa) for c, b in zip(child, blen)]
    argv = ['--dataset', 'primate_data_wang', '--n_particles', '16', '--num_epoch', '1', '--batch_size', '512', '--jcmodel', 'true',
            '--seed', '2', '--score_opt', 'true']

    def run(extra, tmp):
        path = os.path.join(tmp, 'trees.nwk')
        with open(path, 'w') as f:
            f.write('\n'.join(newicks) + '\n')
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'runner.py')] + argv + ['--score_trees', path] + extra, cwd=tmp,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        (res,) = glob.glob(os.path.join(tmp, 'results', '*', '*', '*', '*', 'tree_scores.json'))
        here = os.path.dirname(res)
        files = {}
        for name in sorted(os.listdir(here)):
            if name.endswith(('.json', '.nwk', '.txt', '.fa', '.tre')):
                with open(os.path.join(here, name), 'rb') as f:
                    files[name] = f.read().replace(tmp.encode(), b'TMP')       # (run_parameters.txt names the tree file's path)
        return files

    with tempfile.TemporaryDirectory() as tmp:
        with_flag = run(['--score_ancestral', '2'], tmp)
    with tempfile.TemporaryDirectory() as tmp:
        without = run([], tmp)
    # without the flag: no new file, no key; every other file byte for byte
    assert 'ancestral.fa' not in without and 'ancestral.json' not in without
    assert b'score_ancestral' not in without['run_parameters.txt'] and b'score_ancestral : 2\n' in with_flag['run_parameters.txt']
    assert with_flag['run_parameters.txt'].replace(b'score_ancestral : 2\n', b'') == without['run_parameters.txt']
    assert set(with_flag) == set(without) | {'ancestral.fa', 'ancestral.json'}
    for name in without:
        if name != 'run_parameters.txt':
            assert with_flag[name] == without[name], name
    # the two files
    scores = json.loads(with_flag['tree_scores.json'])
    res = json.loads(with_flag['ancestral.json'])
    order = np.argsort(-np.array([t['loglik_ml'] for t in scores['trees']]), kind='stable')[:2]
    assert [t['tree'] for t in res['trees']] == [int(t) for t in order]
    records = {}
    for line in with_flag['ancestral.fa'].decode().splitlines():
        if line.startswith('>'):
            head = line[1:]
            records[head] = ''
        else:
            records[head] += line
    assert len(records) == 2 * (N - 1)
    for seq in records.values():
        assert len(seq) == S and set(seq) <= set('ACGT?')
    # ... against a direct call under the model and at the lengths the files name; nodes are matched by their clades
    ml = with_flag['trees_ml.nwk'].decode().split()
    m = scores['model']
    with _ffi.Context(4, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(np.array(m['Q']), np.array(m['pi']), np.full(N - 1, 10.0), np.full(N - 1, 10.0), jc69_closed_form=m['jc69_closed_form'])
        for tree in res['trees']:
            assert tree['newick'] == ml[tree['tree']]
            c, b = TP.newick_to_rows(tree['newick'], taxa)
            ll, state, pmax = ctx.trees_ancestral(c[None], b[None], want_post=False, want_pmax=True)
            assert ll[0] == pytest.approx(tree['loglik'], rel=1e-12)
            sm = A.summarise(pmax[0])
            seqs = A.sequences(state[0])
            by_clade = {tuple(cl): k for k, cl in enumerate(A.node_clades(c, taxa))}
            assert len(tree['nodes']) == N - 1
            for node in tree['nodes']:
                k = by_clade[tuple(node['clade'])]
                assert node['mean_pmax'] == pytest.approx(float(sm['mean_pmax'][k]), rel=1e-12)
                assert node['share_below_0.9'] == pytest.approx(float(sm['share_below'][k]), abs=1e-12)
                assert node['n_nan'] == int(sm['n_nan'][k]) == 0
                assert records['tree%d_node%d clade=%s' % (tree['tree'], node['node'], ','.join(node['clade']))] == seqs[k]
