"""The reverse pass of ONE particle system sharded over several ranks (PHYLO_KEEP_GRAPH on a sharded context,
phylo_sweep_backward / phylo_vi_gradients as collective calls, runner.py --train_parallel sharded).  The rig of
tests/test_gpu_sharded.py: several processes on GPU 0, PHYLO_COMM=hostshm for the host-side collectives, every process under a
time-out.  Every rank must hold the same gradient bits; against the unsharded pass of the same global K and seed and against
oracle/cpu_grad.py the tolerance is tests/test_gpu_grad.py's relative 1e-9 per gradient block."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import cpu_grad as G
from phylo_amd import _ffi, model
from phylo_amd.datasets import load_dataset

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KEYS = ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q')
RTOL = 1e-9
EINVAL, ESTATE = -1, -6                                   # PHYLO_EINVAL, PHYLO_ESTATE (include/phylo_hip.h)


def run_world(world, K, dataset, jc, mode, seeds, extra_env=None, salt=0):
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, PHYLO_RDZV_DIR=tmp, MASTER_PORT=str(29400 + (os.getpid() + salt) % 2000), PHYLO_COMM='hostshm')
        env.update(extra_env or {})
        procs = []
        for r in range(world):
            out = os.path.join(tmp, "g%d.npz" % r)
            cmd = [sys.executable, os.path.join(ROOT, "tests", "_shard_grad_worker.py"), str(r), str(world), str(K), dataset,
                   '1' if jc else '0', mode, ','.join(str(s) for s in seeds), out]
            procs.append((out, subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        outs = []
        for out, p in procs:
            try:
                log, _ = p.communicate(timeout=240)
            except subprocess.TimeoutExpired:
                for _, q in procs:
                    q.kill()
                raise
            assert p.returncode == 0, log.decode()[-3000:]
            outs.append(dict(np.load(out)))
        return outs


def _model(dataset, jc):
    g = load_dataset(dataset)['genome']
    N = g.shape[0]
    Q = model.jc_Q() if jc else model.get_Q(model.init_y_q())
    pi = model.get_stationary_probs(np.zeros(4) + 0.25)
    lam = np.full(N - 1, 10.0)
    return g, Q, pi, lam


def _unsharded(dataset, jc, K, seed):
    g, Q, pi, lam = _model(dataset, jc)
    N, S, _ = g.shape
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, pi, lam, lam, jc69_closed_form=jc)
        out = ctx.sweep(seed, _ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        grad = ctx.sweep_backward()
    return out, grad


def _oracle(dataset, jc, K, seed, ancestors):
    g, Q, pi, lam = _model(dataset, jc)
    N = g.shape[0]
    st = G.forward(g, Q, pi, lam, lam, K, seed, _ffi.FLAGS_DEFAULT)['struct']
    for r in range(1, N - 1):
        st['anc'][r] = ancestors[r - 1].astype(np.int64)
    return G.sweep_grad(g, Q, pi, lam, lam, K, seed, _ffi.FLAGS_DEFAULT, struct=st)


def _close(a, b, key):
    scale = max(np.max(np.abs(b)), 1e-300)
    err = np.max(np.abs(np.asarray(a) - np.asarray(b))) / scale
    assert err < RTOL, (key, err, a, b)


def _check_grad(outs, dataset, jc, K, seeds, oracle=True):
    for s in seeds:
        first = outs[0]
        for o in outs:                                    # the same bits on every rank, and again on the same kept graph
            assert o['logz_%d' % s] == first['logz_%d' % s]
            for k in KEYS:
                assert np.array_equal(o['%s_%d' % (k, s)].view(np.uint64), first['%s_%d' % (k, s)].view(np.uint64)), (k, s)
                assert np.array_equal(o['again_%s_%d' % (k, s)].view(np.uint64), first['%s_%d' % (k, s)].view(np.uint64)), (k, s)
        ref, grad = _unsharded(dataset, jc, K, s)
        assert first['logz_%d' % s] == ref['logZ']         # the sharded sweep is bit-identical to one GPU
        for k in KEYS:
            if jc and k in ('d_pi', 'd_Q'):
                continue
            _close(first['%s_%d' % (k, s)], grad[k], k)
        if oracle:
            orc = _oracle(dataset, jc, K, s, ref['ancestors'])
            for k in ('d_lam_l', 'd_lam_r') + (() if jc else ('d_pi', 'd_Q')):
                _close(first['%s_%d' % (k, s)], orc[k], k)


@pytest.mark.parametrize("world,K,jc", [(2, 64, False), (3, 96, True)])
def test_sharded_gradient_parity(world, K, jc):
    """2 ranks K = 64 (GTR start) and 3 ranks K = 96 (JC69) on primate data, several seeds: every rank's phylo_sweep_backward is
    bit-identical to the others', matches the unsharded pass and the oracle at 1e-9; log Z-hat is bit-identical to one GPU."""
    seeds = [3, 11, 20]
    outs = run_world(world, K, 'primate_data', jc, 'grad', seeds, salt=world)
    _check_grad(outs, 'primate_data', jc, K, seeds)


@pytest.mark.parametrize("form,env", [('eager', {'PHYLO_EAGER_NODES': '1'}), ('collective', {'PHYLO_P2P': '0'}),
                                      ('replicated', {'PHYLO_REPLICATED_BOOK': '1'}), ('no-cache', {'PHYLO_NO_REMOTE_CACHE': '1'}),
                                      ('tiny-cache', {'PHYLO_REMOTE_CACHE_CAP': '2'})])
def test_sharded_gradient_forms(form, env):
    """The forms of the sharded sweep (lazy nodes are the default of the test above) give the same checks."""
    seeds = [5, 8]
    outs = run_world(2, 64, 'primate_data', False, 'grad', seeds, extra_env=env, salt=100 + len(form))
    _check_grad(outs, 'primate_data', False, 64, seeds, oracle=False)


def test_sharded_gradient_after_sweep_node():
    """phylo_sweep_node after a lazy sharded sweep that keeps its graph writes every skipped node into its owner's pool and widens
    the marks; the next reverse pass (the form without marks, which reads every node's row from its owner) gives the gradient of
    the lazy pass on every rank, and both match the unsharded pass (tests/test_gpu_grad.py's after_sweep_node case, sharded)."""
    seeds = [4, 9]
    outs = run_world(2, 64, 'primate_data', False, 'node', seeds, salt=200)
    for s in seeds:
        _, grad = _unsharded('primate_data', False, 64, s)
        for o in outs:
            for k in KEYS:
                assert np.array_equal(o['node_%s_%d' % (k, s)].view(np.uint64), outs[0]['node_%s_%d' % (k, s)].view(np.uint64)), k
                scale = max(np.max(np.abs(o['%s_%d' % (k, s)])), 1e-300)
                assert np.max(np.abs(o['node_%s_%d' % (k, s)] - o['%s_%d' % (k, s)])) / scale < 1e-12, k
                _close(o['node_%s_%d' % (k, s)], grad[k], k)


def test_sharded_steps_are_reproducible():
    """Two whole sequences of sharded training steps (phylo_vi_gradients + Adam) at a fixed world size and transport give the
    same bits; the packed gradients are identical on all ranks and match the unsharded call at 1e-9; phylo_vi_apply leaves
    identical variables everywhere."""
    seeds = [1, 2, 3]
    a = run_world(2, 64, 'primate_data', False, 'vi', seeds, salt=300)
    b = run_world(2, 64, 'primate_data', False, 'vi', seeds, salt=301)
    for o in a + b:
        for i in range(len(seeds)):
            for key in ('grads_%d' % i, 'vars_%d' % i):
                assert np.array_equal(o[key].view(np.uint64), a[0][key].view(np.uint64)), key
            assert o['logz_%d' % i] == a[0]['logz_%d' % i]
    # the first step against the unsharded library call at the same start
    g, Q, pi, lam = _model('primate_data', False)
    N, S, _ = g.shape
    v = np.concatenate([np.full(2 * (N - 1), np.log(10.0)), model.init_y_q().reshape(-1), np.zeros(4)])
    with _ffi.Context(64, N, S) as ctx:
        ctx.set_leaves(g)
        logz, grads, _, _ = ctx.vi_gradients(seeds[0], _ffi.FLAGS_DEFAULT, 1, False, v)
    assert logz == a[0]['logz_0']
    R = N - 1
    for name, sl in (('a_l', slice(0, R)), ('a_r', slice(R, 2 * R)), ('y_q', slice(2 * R, 2 * R + 16)), ('y_station', slice(2 * R + 16, None))):
        _close(a[0]['grads_0'][sl], grads[sl], name)


def test_sharded_refusals_leave_the_context_usable():
    """A twisted sweep that keeps its graph, more than 4096 sites and a backward without a kept graph are refused with their
    documented codes on a sharded context; the next plain sweep is still bit-exact."""
    outs = run_world(2, 64, 'primate_data', False, 'refuse', [7], salt=400)
    g, Q, pi, lam = _model('primate_data', False)
    N, S, _ = g.shape
    with _ffi.Context(64, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, pi, lam, lam)
        ref = ctx.sweep(7)
    for o in outs:
        assert int(o['code_twisted']) == EINVAL
        assert int(o['code_backward']) == ESTATE
        assert int(o['code_wide']) == EINVAL
        assert o['logz'] == ref['logZ']
        k0 = int(o['k0'])
        lw = ref['log_weights'][:, k0:k0 + o['log_weights'].shape[1]]
        assert np.array_equal(o['log_weights'].view(np.uint64), lw.view(np.uint64))


def _run_runner(world, argv, salt):
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, PHYLO_RDZV_DIR=tmp, MASTER_PORT=str(29700 + (os.getpid() + salt) % 800), PHYLO_COMM='hostshm')
        procs = []
        for r in range(world):
            out = os.path.join(tmp, "w%d.npz" % r)
            cmd = [sys.executable, os.path.join(ROOT, "tests", "_runner_worker.py"), str(r), str(world), out, '--'] + argv + \
                  ['--n_gpus', str(world)]
            procs.append((out, subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        res = []
        for out, p in procs:
            try:
                log, _ = p.communicate(timeout=240)
            except subprocess.TimeoutExpired:
                for _, q in procs:
                    q.kill()
                raise
            assert p.returncode == 0, log.decode()[-3000:]
            res.append(dict(np.load(out)))
        if world > 1:
            assert os.path.exists(os.path.join(tmp, 'results', 'results.p'))
        return res


def test_runner_sharded_training():
    """`runner.py --n_gpus 2 --train_parallel sharded` on primate_data_wang, K = 32, 2 epochs, Adam: both ranks end with the same
    bits, ELBOs and rates match one process of the same K at 1e-8, and the run differs from --train_parallel replicas."""
    argv = ['--dataset', 'primate_data_wang', '--n_particles', '32', '--num_epoch', '2', '--batch_size', '256',
            '--optimizer', 'Adam', '--learning_rate', '0.05', '--seed', '4']
    two = _run_runner(2, argv + ['--train_parallel', 'sharded'], 11)
    one = _run_runner(1, argv, 12)[0]
    rep = _run_runner(2, argv, 13)[0]
    for r in two:
        assert np.array_equal(r['elbos'].view(np.uint64), two[0]['elbos'].view(np.uint64))
        assert np.array_equal(r['lam'].view(np.uint64), two[0]['lam'].view(np.uint64))
        np.testing.assert_allclose(r['elbos'], one['elbos'], rtol=1e-8)
        np.testing.assert_allclose(r['lam'], one['lam'], rtol=1e-8)
    assert not np.allclose(two[0]['lam'], rep['lam'], rtol=1e-8)
