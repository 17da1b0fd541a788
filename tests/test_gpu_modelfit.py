"""The model fit on the device: VCSMC.score_trees(optimize=True, fit_model=...) over
phylo_trees_grad_model and phylo_trees_grad on the simulated 8-taxon case of the CPU test, and runner.py --score_model_fit.

Every test here needs Context.trees_grad_model."""
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import treegrad_model_cases as MC
from phylo_amd import treepost as TP
from phylo_amd.datasets import load_dataset
from phylo_amd.vcsmc import VCSMC, default_args
from test_gpu_trees_loglik import bits, random_trees

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "score_opt_parent")


def test_score_trees_fits_the_model():
    """the CPU test's case through VCSMC.score_trees: the objective never falls, is the best tree's score, ends
    within the CPU test's margin of the host run of the same fit (treegrad_model_cases.FIT_OBJECTIVE_HOST, which
    test_treegrad_model_cpu.py asserts), and the context's model is afterwards what it was.  (The function is the project's, with
    no interior maximum over Q: agreement with another climber is shown on the host, under the textbook convention.)"""
    case = MC.fit_case()
    taxa = ['t%d' % i for i in range(case['N'])]
    newicks = [TP.rows_to_newick(c, b, taxa) for c, b in zip(case['child'], case['blen'])]
    v = VCSMC({'taxa': taxa, 'genome': case['g']}, K=4, args=default_args())
    try:
        ctx = v._context()
        child, blen = case['child'], case['blen']
        before = ctx.trees_grad(child, blen, want_curv=True)
        given = v.score_trees(newicks)
        scores, sites = v.score_trees(newicks, want_sites=True, optimize=True, fit_model=('q', 'pi'))
        fit = v.last_model_fit
        hist = np.array(fit['history'])
        print("rounds %d, fit_on %r, objective %.10f -> %.10f (host %.10f)" % (fit['rounds'], fit['fit_on'], fit['objective_start'],
                                                                              fit['objective'], MC.FIT_OBJECTIVE_HOST))
        assert (np.diff(hist) >= 0).all() and hist[0] == fit['objective_start'] and hist[-1] == fit['objective']
        assert fit['fit_on'] == [0] and fit['fit'] == ['q', 'pi']
        assert abs(fit['objective'] - MC.FIT_OBJECTIVE_HOST) <= MC.FIT_MARGIN * abs(MC.FIT_OBJECTIVE_HOST)
        assert scores[0] == pytest.approx(fit['objective'], rel=1e-12)
        assert (np.array(scores) >= np.array(v.last_tree_opt['loglik_given'])).all()
        np.testing.assert_array_equal(bits(v.last_tree_opt['loglik_given']), bits(given))
        np.testing.assert_allclose(np.log(sites).sum(axis=1), scores, rtol=1e-12)
        np.testing.assert_allclose(np.array(fit['Q']).sum(axis=1), 0, atol=1e-15)
        assert abs(sum(fit['pi']) - 1) <= 1e-15
        # the context's model is bit for bit what it was: the same calls give the same bits
        for a, b in zip(ctx.trees_grad(child, blen, want_curv=True), before):
            np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(bits(v.score_trees(newicks)), bits(given))
    finally:
        v.close()


ARGV = ['--dataset', 'primate_data_wang', '--n_particles', '16', '--num_epoch', '1', '--batch_size', '512', '--seed', '2',
        '--score_trees', 'trees.nwk', '--score_opt', 'true', '--tree_tests', '200:1']
FILES = ('tree_scores.json', 'trees_ml.nwk', 'tree_tests.json', 'run_parameters.txt')


def run_runner(extra, tmp):
    """runner.py in a process of its own (tests/_runner_worker.py: python's RNG seeded, results under tmp/results)"""
    with open(os.path.join(GOLDEN, 'trees.nwk')) as f:
        text = f.read()
    with open(os.path.join(tmp, 'trees.nwk'), 'w') as f:
        f.write(text)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_runner_worker.py'), '0', '1', os.path.join(tmp, 'out.npz'), '--'] + ARGV + extra,
                       cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    return {os.path.basename(f): open(f, 'rb').read() for f in glob.glob(os.path.join(tmp, 'results', '*'))}


def test_runner_model_fit_and_the_run_without_it():
    """With --score_model_fit: model_ml.json, and loglik_ml of the fit_on tree at or above its --score_opt value.  Without it: the
    score-tree files byte for byte what the parent commit's run of the same command wrote (tests/golden/score_opt_parent,
    recorded from that commit's library and Python files on an MI355X)."""
    with tempfile.TemporaryDirectory() as tmp:
        plain = run_runner([], tmp)
    assert 'model_ml.json' not in plain
    for name in FILES:
        with open(os.path.join(GOLDEN, name), 'rb') as f:
            assert plain[name] == f.read(), name
    with tempfile.TemporaryDirectory() as tmp:
        fitted = run_runner(['--score_model_fit', 'q+pi'], tmp)
    mdl = json.loads(fitted['model_ml.json'])
    scores, base = json.loads(fitted['tree_scores.json']), json.loads(plain['tree_scores.json'])
    t = mdl['fit_on'][0]
    assert mdl['fit_on'] == [int(np.argmax([x['loglik_ml'] for x in base['trees']]))]
    # the first climb IS --score_opt's (which records, of two values it cannot tell apart, the larger: treeopt.NOISE = 2^-46)
    assert mdl['objective_start'] == pytest.approx(base['trees'][t]['loglik_ml'], rel=2.0 ** -46)
    assert scores['trees'][t]['loglik_ml'] >= base['trees'][t]['loglik_ml'] and mdl['objective'] >= mdl['objective_start']
    assert scores['trees'][t]['loglik_ml'] == pytest.approx(mdl['objective'], rel=1e-12)
    assert [x['loglik'] for x in scores['trees']] == [x['loglik'] for x in base['trees']]   # the given trees under the given model
    assert scores['model'] == base['model']                                  # ... which tree_scores.json still names
    assert np.array(mdl['Q']).shape == (4, 4) and len(mdl['pi']) == 4 and np.array(mdl['y_q']).shape == (4, 4) and len(mdl['y_station']) == 4
    assert mdl['rounds'] >= 1 and b'score_model_fit : q+pi' in fitted['run_parameters.txt']
    tests = json.loads(fitted['tree_tests.json'])
    assert tests['obs'] == pytest.approx([x['loglik_ml'] for x in scores['trees']], rel=1e-9)   # the tests ran under the fitted model
    taxa = [str(x) for x in load_dataset('primate_data_wang')['taxa']]
    ml = [line for line in fitted['trees_ml.nwk'].decode().splitlines() if line.strip()]
    assert len(ml) == len(scores['trees']) == 3 and all(TP.newick_to_rows(nw, taxa)[0].shape == (len(taxa) - 1, 2) for nw in ml)
