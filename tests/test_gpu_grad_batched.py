"""The reverse pass of a batched sweep (phylo_sweep_backward_batch, phylo_vi_gradients_batch): G independent particle systems
behind one set of launches, kept for the reverse pass, G gradients out.

Reference and tolerance are those of tests/test_gpu_grad.py, per group: oracle/cpu_grad.py's forward / sweep_grad of K/G particles
with seeds[g] on the device's ancestors of group g, relative 1e-9 of the largest entry of each gradient block and
|d logZ| < 1e-9 max(1, |logZ|).  The forward sweep stays bit-exact: keeping the graph changes no bit of the batch, and group g is
the solo sweep of K/G particles with seeds[g]."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from oracle import cpu_grad as G
from oracle import cpu_ref as O
from phylo_amd import _ffi, train
from phylo_amd.datasets import load_dataset
from tests.test_gpu_grad import RTOL, _codes_genome, _model

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KEYS = ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q')
ARRAYS = ('log_weights', 'log_likelihood', 'left_branches', 'right_branches', 'ancestors', 'merges')


def _codes():
    """the library's error codes by name (include/phylo_hip.h)"""
    import re
    text = open(os.path.join(ROOT, 'include', 'phylo_hip.h')).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r'\b(PHYLO_E[A-Z]+)\s*=\s*(-?\d+)', text)}


def _batch(ctx, seeds, flags):
    ctx.sweep_batch_async(seeds, flags)
    out = ctx.sweep_fetch()
    out['logZ_groups'] = ctx.sweep_fetch_logz(len(seeds))
    return out


def _check_batch(genome, Q, pi, ll, lr, Kg, seeds, flags=_ffi.FLAGS_DEFAULT, jc=False, oracle_groups=None, solo=True):
    """Checks 1-3 of the module for one case; returns the batch's gradients (with 'backward_lists') and the fetched sweep."""
    N, S, _ = genome.shape
    Gn = len(seeds)
    with _ffi.Context(Kg * Gn, N, S) as ctx:
        ctx.set_leaves(genome)
        ctx.set_model(Q, pi, ll, lr, jc69_closed_form=jc)
        plain = _batch(ctx, seeds, flags)
        out = _batch(ctx, seeds, flags | _ffi.KEEP_GRAPH)
        for key in ARRAYS:                                  # keeping the graph does not change a bit of the batch
            assert np.array_equal(plain[key], out[key]), key
        assert np.array_equal(plain['logZ_groups'], out['logZ_groups'])
        g = ctx.sweep_backward_batch(Gn)
        g2 = ctx.sweep_backward_batch(Gn)                   # deterministic, and repeatable on the kept graph
        for key in KEYS:
            assert g[key].shape[0] == Gn
            assert np.array_equal(g[key], g2[key]), key
    if solo:                                                # group g is the sweep of K/G particles with seeds[g]
        with _ffi.Context(Kg, N, S) as one:
            one.set_leaves(genome)
            one.set_model(Q, pi, ll, lr, jc69_closed_form=jc)
            for gi, sd in enumerate(seeds):
                alone = one.sweep(int(sd), flags)
                cols = slice(gi * Kg, (gi + 1) * Kg)
                for key in ARRAYS:
                    assert np.array_equal(out[key][:, cols], alone[key]), (key, gi)
                assert out['logZ_groups'][gi] == alone['logZ'], gi
    for gi in (range(Gn) if oracle_groups is None else oracle_groups):
        sd = int(seeds[gi])
        f = G.forward(genome, Q, pi, ll, lr, Kg, sd, flags)
        st = f['struct']
        for r in range(1, N - 1):
            st['anc'][r] = out['ancestors'][r - 1][gi * Kg:(gi + 1) * Kg].astype(np.int64)
        ref = G.sweep_grad(genome, Q, pi, ll, lr, Kg, sd, flags, struct=st)
        z = out['logZ_groups'][gi]
        assert abs(ref['logZ'] - z) < 1e-9 * max(1.0, abs(z)), gi
        for key in ('d_lam_l', 'd_lam_r') + (() if jc else ('d_pi', 'd_Q')):
            scale = max(np.max(np.abs(ref[key])), 1e-300)
            err = np.max(np.abs(g[key][gi] - ref[key])) / scale
            print('group %d %s rel err %.3e' % (gi, key, err))
            assert err < RTOL, (gi, key, err, g[key][gi], ref[key])
    return g, out


# ---- 2. per-group gradient against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,Kg,Gn,seed", [(5, 70, 32, 2, 1), (6, 70, 64, 3, 2), (7, 300, 32, 5, 3), (8, 300, 64, 2, 4), (8, 70, 32, 3, 5)])
def test_batched_gradient_random_gtr_coded_leaves(N, S, Kg, Gn, seed):
    rng = np.random.default_rng(100 + seed)
    genome = _codes_genome(rng, N, S)
    Q, pi, ll, lr = _model(rng, N)
    _check_batch(genome, Q, pi, ll, lr, Kg, [1000 * seed + 7 * i + 1 for i in range(Gn)])


@pytest.mark.parametrize("N,S,Kg,Gn", [(5, 70, 64, 2), (6, 300, 32, 3)])
def test_batched_gradient_generic_leaves(N, S, Kg, Gn):
    rng = np.random.default_rng(13 + N)
    genome = rng.uniform(0.05, 1.0, size=(N, S, 4))
    Q, pi, ll, lr = _model(rng, N)
    _check_batch(genome, Q, pi, ll, lr, Kg, [3 + 11 * i for i in range(Gn)])


def test_batched_gradient_jc69_rates_only():
    genome = load_dataset('primate_data_wang')['genome'][:, :70]
    N = genome.shape[0]
    lam = np.full(N - 1, 10.0)
    _check_batch(genome, O.jc_Q(), np.full((1, 4), 0.25), lam, lam, 32, [8, 9, 10], jc=True)


def test_batched_gradient_q1_quirk_off():
    rng = np.random.default_rng(12)
    genome = _codes_genome(rng, 7, 300)
    Q, pi, ll, lr = _model(rng, 7)
    _check_batch(genome, Q, pi, ll, lr, 64, [5, 6, 7, 8, 9], flags=0)


def test_batched_gradient_primate_subset():
    """The reference's initial model on real sites, K/G = 256, G = 4."""
    genome = load_dataset('primate_data')['genome'][:8, :200]
    N = genome.shape[0]
    Q = np.full((4, 4), 1.0 / 3.0)
    np.fill_diagonal(Q, -1.0)
    pi = np.full((1, 4), 0.25)
    lam = np.full(N - 1, 10.0)
    _check_batch(genome, Q, pi, lam, lam, 256, [2024, 2025, 2026, 2027])


def test_batched_gradient_flat_weights_many_adopted_nodes():
    """All-gap rows: every particle has the same weight, the resampling keeps most lineages, most nodes are adopted."""
    rng = np.random.default_rng(21)
    genome = np.ones((6, 70, 4))
    Q, pi, ll, lr = _model(rng, 6)
    _check_batch(genome, Q, pi, ll, lr, 64, [31, 32, 33])


def test_batched_gradient_total_k_beyond_one_sort_takes_device_lists():
    """Total K = 10240 > 8192 with K/G = 512: the device builders sort per (rank event, group) and apply."""
    rng = np.random.default_rng(22)
    genome = _codes_genome(rng, 5, 40)
    Q, pi, ll, lr = _model(rng, 5)
    g, _ = _check_batch(genome, Q, pi, ll, lr, 512, list(range(50, 70)), oracle_groups=(0, 7, 19), solo=False)
    assert g['backward_lists'] == 'device'


# ---- 4. one group ---------------------------------------------------------------------------------------------------------------
def test_one_group_batch_is_the_single_pass():
    rng = np.random.default_rng(23)
    genome = _codes_genome(rng, 7, 120)
    Q, pi, ll, lr = _model(rng, 7)
    flags = _ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH
    with _ffi.Context(128, 7, 120) as ctx:
        ctx.set_leaves(genome)
        ctx.set_model(Q, pi, ll, lr)
        ctx.sweep_async(41, flags)
        single = ctx.sweep_backward()
        z1 = ctx.sweep_fetch(arrays=False)['logZ']
        ctx.sweep_batch_async([41], flags)
        batch = ctx.sweep_backward_batch(1)
        zb = ctx.sweep_fetch_logz(1)
        ctx.sweep_async(41, flags)                          # the batch call after the unbatched sweep too
        batch2 = ctx.sweep_backward_batch(1)
        v = train.Variables(7, np.log(10.0), False)
        z3, g3, _, _ = ctx.vi_gradients(41, _ffi.FLAGS_DEFAULT, 1, False, v.pack())
        z4, g4, _, _ = ctx.vi_gradients_batch([41], _ffi.FLAGS_DEFAULT, False, v.pack())
    assert zb[0] == z1
    for key in KEYS:
        assert np.array_equal(batch[key][0], single[key]), key
        assert np.array_equal(batch2[key][0], single[key]), key
    assert z4[0] == z3 and np.array_equal(g4[0], g3)


# ---- 5. forms -------------------------------------------------------------------------------------------------------------------
def _grads_under(monkeypatch, env, genome, model, Kg, seeds):
    for name in ('PHYLO_GRAD_ROWS_CHAIN', 'PHYLO_GRAD_COEFF_CHAIN', 'PHYLO_GRAD_ONE_STREAM', 'PHYLO_REV_HOST_LISTS'):
        monkeypatch.delenv(name, raising=False)
    if env:
        monkeypatch.setenv(env, '1')                        # (read when the context is created)
    N, S, _ = genome.shape
    with _ffi.Context(Kg * len(seeds), N, S) as ctx:
        ctx.set_leaves(genome)
        ctx.set_model(*model)
        ctx.sweep_batch_async(seeds, _ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        return ctx.sweep_backward_batch(len(seeds))


@pytest.mark.parametrize("N,S,Kg,Gn", [(6, 70, 64, 3), (8, 300, 256, 4)])
def test_forms_of_the_batched_pass_agree(monkeypatch, N, S, Kg, Gn):
    rng = np.random.default_rng(24 + N)
    genome = _codes_genome(rng, N, S)
    model = _model(rng, N)
    seeds = [61 + i for i in range(Gn)]
    base = _grads_under(monkeypatch, None, genome, model, Kg, seeds)
    assert base['backward_lists'] == 'device'
    for env in ('PHYLO_GRAD_ROWS_CHAIN', 'PHYLO_GRAD_COEFF_CHAIN', 'PHYLO_GRAD_ONE_STREAM'):
        other = _grads_under(monkeypatch, env, genome, model, Kg, seeds)
        for key in KEYS:
            assert np.array_equal(other[key], base[key]), (env, key)
    host = _grads_under(monkeypatch, 'PHYLO_REV_HOST_LISTS', genome, model, Kg, seeds)
    assert host['backward_lists'] == 'host'
    for key in KEYS:                                        # (the host builders order a node's flagged parents differently)
        for gi in range(Gn):
            scale = max(np.max(np.abs(base[key][gi])), 1e-300)
            err = np.max(np.abs(host[key][gi] - base[key][gi])) / scale
            assert err < RTOL, (key, gi, err)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    codes = _codes()
    EINVAL, ESTATE = codes['PHYLO_EINVAL'], codes['PHYLO_ESTATE']
    rng = np.random.default_rng(25)
    genome = _codes_genome(rng, 5, 40)
    Q, pi, ll, lr = _model(rng, 5)
    keep = _ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH
    with _ffi.Context(96, 5, 40) as ctx:
        ctx.set_leaves(genome)
        ctx.set_model(Q, pi, ll, lr)
        with pytest.raises(_ffi.PhyloError) as e:           # twisted batch with graph
            ctx.sweep_batch_async([1, 2, 3], keep | _ffi.TWISTING)
        assert e.value.code == EINVAL and 'TWISTING' in str(e.value)
        ctx.sweep_batch_async([1, 2, 3], _ffi.FLAGS_DEFAULT)
        with pytest.raises(_ffi.PhyloError) as e:           # batch backward without a kept graph
            ctx.sweep_backward_batch(3)
        assert e.value.code == ESTATE
        ctx.sweep_batch_async([1, 2, 3], keep)
        with pytest.raises(_ffi.PhyloError) as e:           # the single form after G = 3
            ctx.sweep_backward()
        assert e.value.code == ESTATE and 'phylo_sweep_backward_batch' in str(e.value)
        with pytest.raises(_ffi.PhyloError) as e:           # a wrong G
            ctx.sweep_backward_batch(2)
        assert e.value.code == EINVAL
        g = ctx.sweep_backward_batch(3)                     # the refused calls left the graph alone
        assert np.isfinite(g['d_lam_l']).all()
    big = np.ones((4, 4100, 4))
    with _ffi.Context(16, 4, 4100) as ctx:                  # S > 4096 batch with graph
        ctx.set_leaves(big)
        ctx.set_model(O.jc_Q(), np.full((1, 4), 0.25), np.full(3, 10.0), np.full(3, 10.0))
        with pytest.raises(_ffi.PhyloError) as e:
            ctx.sweep_batch_async([1, 2], keep)
        assert e.value.code == EINVAL and '4096' in str(e.value)
        ctx.sweep_batch_async([1, 2], _ffi.FLAGS_DEFAULT)   # ... which the batch without the graph still runs
        assert np.isfinite(ctx.sweep_fetch_logz(2)).all()


# ---- 7. trainer -----------------------------------------------------------------------------------------------------------------
def _trainer(genome, K, opt_name, native, batched, lr=0.01):
    N = genome.shape[0]
    v = train.Variables(N, np.log(10.0), False)
    rng = np.random.default_rng(5)
    v.a_l = v.a_l + rng.normal(size=N - 1) * 0.2
    v.a_r = v.a_r + rng.normal(size=N - 1) * 0.2
    v.y_q = np.asarray(v.y_q, dtype=np.float64) + rng.normal(size=(4, 4)) * 0.2
    v.y_station = v.y_station + rng.normal(size=4) * 0.2
    return train.Trainer(genome, K, v, train.make_optimizer(opt_name, lr), genome.shape[1], native=native, batched=batched)


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("opt_name", ['GradientDescentOptimizer', 'Adam'])
def test_trainer_batched_equals_serial(native, opt_name):
    genome = load_dataset('primate_data')['genome'][:7, :160]
    sites = np.arange(160)
    tb = _trainer(genome, 64, opt_name, native, 3)
    ts = _trainer(genome, 64, opt_name, native, 1)
    try:
        assert tb.ctx.K == 192 and ts.ctx.K == 64
        seeds = lambda i: (900 + i, (900 + i + (1 << 32), 900 + i + (2 << 32)))
        cb = tb.step(sites, *seeds(0))
        cs = ts.step(sites, *seeds(0))
        assert cb == cs                                     # the forward is bit-exact and the mean's order the same
        for name in tb.last['grads']:
            a, b = np.asarray(tb.last['grads'][name]), np.asarray(ts.last['grads'][name])
            assert np.max(np.abs(a - b)) <= RTOL * max(np.max(np.abs(b)), 1e-300), name
        with pytest.raises(ValueError):
            tb.step(sites, 1, (2,))                         # batched=3 steps over three seeds
        if opt_name == 'GradientDescentOptimizer':
            for i in range(1, 4):
                tb.step(sites, *seeds(i))
                ts.step(sites, *seeds(i))
            pb, ps = tb.v.pack(), ts.v.pack()
            assert np.max(np.abs(pb - ps) / np.maximum(np.abs(ps), 1e-300)) < 1e-8
    finally:
        tb.close()
        ts.close()


# ---- 8. runner ------------------------------------------------------------------------------------------------------------------
def _run(argv, tmp_path, monkeypatch):
    import runner
    from phylo_amd.vcsmc import VCSMC
    monkeypatch.chdir(tmp_path)
    random.seed(7)                                          # (the site minibatches come from python's global RNG)
    np.random.seed(7)
    args = runner.parse_args(argv)
    vc = VCSMC(load_dataset(args.dataset, ambiguity=args.ambiguity), K=args.n_particles, args=args)
    elbos = vc.train(epochs=args.num_epoch, batch_size=args.batch_size, learning_rate=args.learning_rate,
                     memory_optimization=args.memory_optimization, save_dir=None)
    return np.asarray(elbos), list(vc.minibatch_costs)


def test_runner_grad_batched(tmp_path, monkeypatch, capsys):
    base = ['--dataset', 'primate_data_wang', '--n_particles', '32', '--grad_samples', '3', '--num_epoch', '2', '--batch_size', '128']
    eb, cb = _run(base + ['--grad_batched', 'true'], tmp_path, monkeypatch)
    es, cs = _run(base, tmp_path, monkeypatch)
    assert len(eb) == 2 and np.isfinite(eb).all() and len(cb) == len(cs) and len(cb) >= 2
    assert cb[0] == cs[0]
    import runner
    monkeypatch.chdir(tmp_path)
    elbos = runner.main(base + ['--grad_batched', 'true', '--num_epoch', '1'])     # the CLI's own path, artefacts included
    assert np.isfinite(elbos).all()
    for extra, word in ((['--nested', 'true'], '--nested'), (['--train_parallel', 'sharded'], 'sharded')):
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'runner.py')] + base + ['--grad_batched', 'true'] + extra, cwd=str(tmp_path),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        text = p.stdout.decode()
        assert p.returncode != 0 and '--grad_batched' in text and word in text, text
