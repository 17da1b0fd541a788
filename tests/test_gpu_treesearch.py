"""NNI search on the device: phylo_amd.treesearch.nni_search over Context.trees_grad and
Context.trees_nni on the 8-taxon case whose reference-only run test_treenni_cpu.py holds clear of every close decision, and
VCSMC.score_trees(search='nni').

Every test here needs Context.trees_nni: AttributeError without it."""
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import treenni_cases as NC
from phylo_amd.datasets import load_dataset
from phylo_amd.treepost import rows_to_newick
from phylo_amd.vcsmc import VCSMC, default_args
from test_gpu_trees_loglik import make_ctx, random_trees
from test_treenni_cpu import run_search

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_search_on_the_device_takes_the_reference_runs_moves():
    g, Q, prior, child, blen, c0 = NC.search_case()
    want = NC.clades(c0)
    ref, _, _ = run_search(*NC.reference_fns(g, Q, prior), child, blen)
    with make_ctx(g, Q, pi=prior) as ctx:
        out, gap, off = run_search(lambda c, b: ctx.trees_grad(c, b, want_curv=True), ctx.trees_nni, child, blen)
    print("moves", out['moves'], "rounds", out['rounds'], "margins %.3g %.3g" % (gap, off))
    assert out['moves'] == ref['moves'] and out['converged'].all()
    np.testing.assert_array_equal(out['child'], ref['child'])
    np.testing.assert_array_equal(out['rounds'], ref['rounds'])
    for t in range(child.shape[0]):
        assert NC.clades(out['child'][t]) == want, t
        assert (np.diff(out['history'][t]) >= 0).all()
    np.testing.assert_allclose(out['loglik'], ref['loglik'], rtol=1e-9)


def test_score_trees_with_search():
    d = load_dataset('primate_data_wang')                                  # primates_small
    taxa = [str(t) for t in d['taxa']]
    child, blen = random_trees(len(taxa), 12, 3)
    newicks = [rows_to_newick(c, b + 0.02, taxa) for c, b in zip(child, blen)]
    v = VCSMC(d, K=16, args=default_args(jcmodel=True, seed=2))
    ml = v.score_trees(newicks, optimize=True)
    found, sites = v.score_trees(newicks, optimize=True, search='nni', search_rounds=4, want_sites=True)
    info = v.last_tree_search
    print("ML lengths", ml, "after the search", found, "moves", info['nni_moves'], "rounds", info['rounds'])
    assert len(found) == 3 and sites.shape == (3, d['genome'].shape[1]) and len(info['newicks']) == 3
    for a, b, m in zip(ml, found, info['loglik_ml']):
        assert b >= a and m == pytest.approx(a, rel=1e-9)
    assert any(n > 0 for n in info['nni_moves'])                           # random trees over real data: some move pays
    again = v.score_trees(info['newicks'])                                 # the trees found, scored as given
    np.testing.assert_allclose(again, found, rtol=1e-12)                   # (rows_to_newick writes lengths that read back bit for bit)
    with pytest.raises(ValueError):
        v.score_trees(newicks, search='nni')


def test_runner_score_search():
    """runner.py --score_search nni:2: trees_search.nwk beside trees_ml.nwk, the search's fields in tree_scores.json, the tests on
    the trees found"""
    d = load_dataset('primate_data_wang')
    taxa = [str(t) for t in d['taxa']]
    child, blen = random_trees(len(taxa), 12, 3)
    argv = ['--dataset', 'primate_data_wang', '--n_particles', '16', '--num_epoch', '1', '--batch_size', '512', '--jcmodel', 'true',
            '--seed', '2', '--score_opt', 'true', '--score_search', 'nni:2', '--tree_tests', '200:1']
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
    assert len(found) == 3 and len(ml) == 3 and len(scores['trees']) == 3
    for t, obs in zip(scores['trees'], tests['obs']):
        assert t['loglik_search'] >= t['loglik_ml'] >= t['loglik'] and 0 <= t['nni_moves'] <= t['search_rounds'] <= 2
        assert obs == pytest.approx(t['loglik_search'], rel=1e-9)           # the tests ran on the trees found
    assert any(t['nni_moves'] > 0 for t in scores['trees']) and found != ml
