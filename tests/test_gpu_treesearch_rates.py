"""NNI search under rate mixtures on the device: phylo_amd.treesearch.nni_search over
Context.trees_grad_rates and Context.trees_nni_rates on the 8-taxon case whose restatement-only run test_treenni_rates_cpu.py holds
clear of every close decision; VCSMC.score_trees(rates=..., fit=..., search='nni'); runner.py --score_fit_search.

Every test here needs Context.trees_nni_rates: AttributeError without it."""
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import treenni_cases as NC
import treenni_rates_cases as RC
from phylo_amd import rates as R
from phylo_amd.datasets import load_dataset
from phylo_amd.treepost import rows_to_newick
from phylo_amd.vcsmc import VCSMC, default_args
from test_gpu_trees_loglik import make_ctx, random_trees
from test_treenni_rates_cpu import run_search

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_search_on_the_device_takes_the_restatement_runs_moves():
    g, Q, prior, child, blen, c0 = RC.search_case()
    want = NC.clades(c0)
    rates, weights = RC.SEARCH_MIX
    ref, _, _ = run_search(*RC.reference_fns(g, Q, prior, rates, weights), child, blen, lo=RC.SEARCH_LO)
    with make_ctx(g, Q, pi=prior) as ctx:
        out, gap, off = run_search(lambda c, b: ctx.trees_grad_rates(c, b, rates, weights, want_curv=True),
                                   lambda c, b: ctx.trees_nni_rates(c, b, rates, weights), child, blen, lo=RC.SEARCH_LO)
        # the same search with every tree under its own copy of the mixture, following it by index: the same moves and bits
        rt, wt = np.tile(rates, (4, 1)), np.tile(weights, (4, 1))
        own = run_search(lambda c, b, i: ctx.trees_grad_rates(c, b, rt[i], wt[i], want_curv=True),
                         lambda c, b, i: ctx.trees_nni_rates(c, b, rt[i], wt[i]), child, blen, lo=RC.SEARCH_LO, with_index=True)[0]
    print("moves", out['moves'], "rounds", out['rounds'], "margins %.3g %.3g" % (gap, off))
    assert out['moves'] == ref['moves'] and out['converged'].all()
    np.testing.assert_array_equal(out['child'], ref['child'])
    np.testing.assert_array_equal(out['rounds'], ref['rounds'])
    for t in range(child.shape[0]):
        assert NC.clades(out['child'][t]) == want, t
        assert (np.diff(out['history'][t]) >= 0).all()
    np.testing.assert_allclose(out['loglik'], ref['loglik'], rtol=1e-9)
    assert own['moves'] == out['moves']
    np.testing.assert_array_equal(own['loglik'].view(np.uint64), out['loglik'].view(np.uint64))


def test_score_trees_with_fit_and_search():
    d = load_dataset('primate_data_wang')                                  # primates_small
    taxa = [str(t) for t in d['taxa']]
    child, blen = random_trees(len(taxa), 12, 3)
    newicks = [rows_to_newick(c, b + 0.02, taxa) for c, b in zip(child, blen)]
    v = VCSMC(d, K=16, args=default_args(jcmodel=True, seed=2))
    spec = R.parse_spec('gamma:1.0:4')
    ml = v.score_trees(newicks, rates=spec, optimize=True, fit=('alpha',))
    found, sites = v.score_trees(newicks, rates=spec, optimize=True, fit=('alpha',), search='nni', search_rounds=3, want_sites=True)
    info, opt = v.last_tree_search, v.last_tree_opt
    print("ML", ml, "after the search", found, "moves", info['nni_moves'], "rounds", info['rounds'], "alpha", opt['alpha'], "->", info['alpha'])
    assert len(found) == 3 and sites.shape == (3, d['genome'].shape[1]) and len(info['newicks']) == 3
    for a, b, m in zip(ml, found, info['loglik_ml']):
        assert b >= a and m == pytest.approx(a, rel=1e-9)                  # found >= ml per tree
    assert all(0.02 <= a <= 100.0 for a in info['alpha']) and info['pinv'] is None
    assert all(0 <= n <= r <= 3 for n, r in zip(info['nni_moves'], info['rounds']))
    for t in range(3):                                                     # the trees found, scored as given under their final mixtures
        again = v.score_trees([info['newicks'][t]], rates=R.rate_model(info['alpha'][t], 4))
        np.testing.assert_allclose(again, [found[t]], rtol=1e-12)
    shared = v.score_trees(newicks, rates=spec, optimize=True, search='nni', search_rounds=2)      # without fit: the shared mixture
    plain = v.score_trees(newicks, rates=spec, optimize=True)
    assert all(b >= a for a, b in zip(plain, shared)) and 'alpha' not in v.last_tree_search
    with pytest.raises(ValueError):
        v.score_trees(newicks, rates=spec, search='nni')


def test_runner_score_fit_search():
    """runner.py --score_fit branches+alpha --score_fit_search nni:2 in a child process: trees_search.nwk beside trees_ml.nwk, the
    search's fields and the final alpha in tree_scores.json, the tests on the trees found"""
    d = load_dataset('primate_data_wang')
    taxa = [str(t) for t in d['taxa']]
    child, blen = random_trees(len(taxa), 12, 3)
    argv = ['--dataset', 'primate_data_wang', '--n_particles', '16', '--num_epoch', '1', '--batch_size', '512', '--jcmodel', 'true',
            '--seed', '2', '--score_rates', 'gamma:1.0:4', '--score_fit', 'branches+alpha', '--score_fit_search', 'nni:2',
            '--tree_tests', '200:1']
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'trees.nwk')
        with open(path, 'w') as f:
            f.write('\n'.join(rows_to_newick(c, b + 0.02, taxa) for c, b in zip(child, blen)) + '\n')
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'runner.py')] + argv + ['--score_trees', path], cwd=tmp,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        (res,) = glob.glob(os.path.join(tmp, 'results', '*', '*', '*', '*', 'tree_scores.json'))
        here = os.path.dirname(res)
        with open(res) as f:
            scores = json.load(f)
        with open(os.path.join(here, 'trees_search.nwk')) as f:
            found = [line.strip() for line in f if line.strip()]
        with open(os.path.join(here, 'trees_ml.nwk')) as f:
            ml = [line.strip() for line in f if line.strip()]
        with open(os.path.join(here, 'tree_tests.json')) as f:
            tests = json.load(f)
        with open(os.path.join(here, 'run_parameters.txt')) as f:
            assert "score_fit_search : ('nni', 2)" in f.read()
    assert len(found) == 3 and len(ml) == 3 and len(scores['trees']) == 3 and scores['rates']['spec'] == 'gamma:1.0:4'
    for t, obs in zip(scores['trees'], tests['obs']):
        assert t['loglik_search'] >= t['loglik_ml'] >= t['loglik'] and 0 <= t['nni_moves'] <= t['search_rounds'] <= 2
        assert 0.02 <= t['alpha'] <= 100.0 and 0.02 <= t['alpha_search'] <= 100.0 and 'pinv' not in t and 'pinv_search' not in t
        assert obs == pytest.approx(t['loglik_search'], rel=1e-9)           # the tests ran on the trees found
