"""The reverse pass, the VI step and a training run on alignments of 66 to 130 taxa (a context accepts up to 512): every form the
pass has, any number of consecutive passes on one context.

Above 65 taxa the hand-off between the coefficient launches and pg_nodes_rows_all needs per-rank-event state for more than 64 rank
events: a 64-bit mask aliased rank events 64 and above, and only the first 64 completion tickets were
zeroed per pass, so a SECOND pass on one context could not complete.  The VI entry points refused outright.

Reference and tolerance are those of tests/test_gpu_grad.py: oracle/cpu_grad.py on the device's ancestors, relative 1e-9 of the
largest entry of each gradient block, |d logZ| < 1e-9 max(1, |logZ|).  Inputs: tests/many_taxa_cases.py (seeded).

Rank events and adopters.  Rank event r (0-based, R = N - 1 of them) "has adopters" when some particle of rank event r + 1 adopted
one of its nodes: ancestors[r] is that row, so EVERY rank event r <= R - 2 has adopters (K draws each) and the last one, R - 1,
never has.  With N = 66 the rank events are 0 .. 64 and the only one at or beyond 64 is the last: a rank event r >= 64 WITH
adopters needs N >= 67.  The flat-weights case therefore runs at N = 66 (rank event 64 without adopters: the aliased bit 0 of the
old mask made its workgroups wait for a launch that never comes) and at N = 67 (rank event 64 with adopters, 65 without), and
asserts both conditions from the fetched ancestors where they can hold.

Twisted oracle time, measured on the CPU at N = 66, K = 2, S = 8, M = 1: forward_twisted 12 s, sweep_grad_twisted 48 s, the plain
sweep_grad of _check_twisted 0.1 s -- a minute in all (S = 4 takes the same: the time goes into the 2145 pairs of the first rank
events, not into the sites)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import cpu_grad as G
from phylo_amd import _ffi
from phylo_amd import train as T
from tests.many_taxa_cases import coded_alignment, datadict, random_model
from tests.test_gpu_grad import RTOL, _check, _check_twisted, _device_lists_match_host

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KEYS = ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q')
SWITCHES = ('PHYLO_GRAD_ROWS_CHAIN', 'PHYLO_GRAD_COEFF_CHAIN', 'PHYLO_REV_HOST_LISTS', 'PHYLO_GRAD_ONE_STREAM')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _oracle(genome, Q, pi, ll, lr, K, seed, flags, ancestors):
    N = genome.shape[0]
    st = G.forward(genome, Q, pi, ll, lr, K, seed, flags)['struct']
    for r in range(1, N - 1):
        st['anc'][r] = ancestors[r - 1].astype(np.int64)
    return G.sweep_grad(genome, Q, pi, ll, lr, K, seed, flags, struct=st)


def _assert_oracle(g, logZ, ref, what):
    assert abs(ref['logZ'] - logZ) < 1e-9 * max(1.0, abs(logZ)), what
    for key in KEYS:
        scale = max(np.max(np.abs(ref[key])), 1e-300)
        err = np.max(np.abs(g[key] - ref[key])) / scale
        print('%s %s rel err %.3e' % (what, key, err))
        assert err < RTOL, (what, key, err)


def _assert_same_bits(a, b, what):
    for key in KEYS:
        scale = max(np.max(np.abs(a[key])), 1e-300)
        print('%s %s rel diff %.3e' % (what, key, np.max(np.abs(np.asarray(a[key]) - np.asarray(b[key]))) / scale))
    for key in KEYS:
        assert np.array_equal(_bits(a[key]), _bits(b[key])), (what, key)


def _consecutive_passes(genome, Q, pi, ll, lr, K, seeds, flags=_ffi.FLAGS_DEFAULT, passes=3):
    """On ONE context, per seed: a sweep that keeps its graph and `passes` reverse passes -- all with the same bits, and within RTOL
    of the oracle.  Returns per seed (fetched sweep, gradient)."""
    N, S, _ = genome.shape
    runs = []
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(genome)
        ctx.set_model(Q, pi, ll, lr)
        for seed in seeds:
            out = ctx.sweep(seed, flags | _ffi.KEEP_GRAPH)
            gs = [ctx.sweep_backward() for _ in range(passes)]
            runs.append((seed, out, gs))
    res = []
    for seed, out, gs in runs:
        for i, g in enumerate(gs[1:]):
            _assert_same_bits(gs[0], g, 'seed %d pass %d against pass 0' % (seed, i + 1))
        assert all(np.all(np.isfinite(gs[0][key])) for key in KEYS)
        _assert_oracle(gs[0], out['logZ'], _oracle(genome, Q, pi, ll, lr, K, seed, flags, out['ancestors']), 'N %d seed %d' % (N, seed))
        res.append((out, gs[0]))
    return res


# ---- 1. plain proposal, default forms: consecutive passes on one context (the ticket reset) ----------------------------------------
@pytest.mark.parametrize("N,S,K", [(66, 40, 24), (67, 130, 64), (100, 24, 32), (130, 24, 16)])
def test_three_consecutive_passes_and_a_fresh_sweep_on_one_context(N, S, K):
    """Three consecutive phylo_sweep_backward calls on one context are bit-identical and match the oracle; a fresh sweep (another
    seed) followed by three more passes on the same context does so again."""
    genome = coded_alignment(1000 + N, N, S)
    Q, pi, ll, lr = random_model(2000 + N, N)
    (_, g0), _ = _consecutive_passes(genome, Q, pi, ll, lr, K, seeds=(12, 13))
    assert g0['backward_lists'] == 'device'                 # the default after a lazy plain sweep: the form with the hand-off


# ---- 2. the same gradient bits across forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", SWITCHES + ('PHYLO_EAGER_NODES',))
@pytest.mark.parametrize("N,S,K", [(66, 40, 24), (100, 24, 32)])
def test_same_gradient_bits_across_forms(monkeypatch, N, S, K, switch):
    """One context per setting (the switches are read when the context is created; PHYLO_EAGER_NODES is a sweep flag): the default's
    gradient bits under every switch, each within RTOL of the oracle (_check).

    PHYLO_REV_HOST_LISTS and PHYLO_EAGER_NODES once differed from the default in the last place (at most 4.8e-16 of a block's largest
    entry at these sizes; tests/test_gpu_grad.py holds them to 1e-12): the host builders leave a node's flagged parents descending
    where the device builders leave them ascending, and a sweep that stored every node left no marks, so its pass took other
    kernels.  Above 65 taxa -- where no reverse pass worked before, so no gradient has bits to keep -- the pass turns the host-built
    tails round and writes the marks of such a sweep from its ancestors: the same sums in the same order
    in every form.  Up to 65 taxa each form keeps the bits it had, and tests/test_gpu_grad.py goes on covering the form without
    marks with the plain proposal."""
    genome = coded_alignment(1000 + N, N, S)
    Q, pi, ll, lr = random_model(2000 + N, N)
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    g = _check(genome, Q, pi, ll, lr, K=K, seed=12)[0]
    flags = _ffi.FLAGS_DEFAULT
    if switch == 'PHYLO_EAGER_NODES':
        flags |= _ffi.EAGER_NODES
    else:
        monkeypatch.setenv(switch, '1')
    g_sw = _check(genome, Q, pi, ll, lr, K=K, seed=12, flags=flags)[0]
    _assert_same_bits(g, g_sw, 'N %d %s' % (N, switch))


# ---- 3. flat weights: many adopted nodes on both sides of rank event 64 --------------------------------------------------------------
@pytest.mark.parametrize("N", [66, 67])
def test_flat_weights_adopters_on_both_sides_of_rank_event_64(N):
    """np.ones leaves (all-gap rows: the data say nothing, the weights are the proposal's and the prior's alone; see the module
    docstring for which rank events can have adopters).  Asserted from the fetched ancestors, not assumed.  With K = 24 between 1
    and 16 nodes of every rank event but the last are adopted.

    "At least one rank event has none": by construction that is the last rank event and no other -- every particle of rank event
    r + 1 adopts a node of rank event r, whatever the weights, so no peaked-weights case can empty an interior one.  Nothing about
    it can be asserted from the ancestors (they have no row for it); what IS checked is that the pass over a last rank event at or
    beyond 64 completes three times on one context (N = 66: rank event 64, the case whose aliased mask bit made its workgroups
    wait for a launch that never comes), and that every interior rank event's row is there and in range."""
    S, K = 40, 24
    genome = np.ones((N, S, 4))
    Q, pi, ll, lr = random_model(2000 + N, N)
    (out, _), _ = _consecutive_passes(genome, Q, pi, ll, lr, K, seeds=(3, 4))
    anc = out['ancestors']                                  # row r: the nodes of rank event r that rank event r + 1 adopted
    R = N - 1
    assert anc.shape == (R - 1, K)
    adopted = [np.unique(anc[r]).size for r in range(R - 1)] + [0]   # per rank event; the last has no row: nobody adopts it
    print('N %d adopted nodes per rank event: %s' % (N, adopted))
    assert min(adopted[:R - 1]) >= 1                        # every rank event but the last has adopted nodes
    assert anc.min() >= 0 and anc.max() < K
    assert R - 1 >= 64                                      # the last rank event, the one without adopters, is at or beyond 64
    assert any(n > 0 for n in adopted[:64])                 # rank events below 64 with adopters
    if N >= 67:
        assert any(n > 0 for n in adopted[64:])             # a rank event r >= 64 WITH adopters (needs N >= 67)


# ---- 4. the device-built lists against the host builders -----------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,K", [(66, 40, 24), (130, 24, 16)])
def test_device_built_lists_equal_the_host_builders(N, S, K):
    Q, pi, ll, lr = random_model(2000 + N, N)
    h, _ = _device_lists_match_host(N, S, K, coded_alignment(1000 + N, N, S), Q, pi, ll, lr, seed=12)
    assert h['n_adp'] > 0 and len(h['ev_adp0']) == N


# ---- 5. the VI step and training -------------------------------------------------------------------------------------------------------
def _variables(rng, N):
    v = T.Variables(N, 1.2, jcmodel=False)
    v.a_l = v.a_l + rng.normal(size=N - 1) * 0.2
    v.a_r = v.a_r + rng.normal(size=N - 1) * 0.2
    v.y_q = rng.normal(size=(4, 4)) * 0.2
    np.fill_diagonal(v.y_q, 0.0)
    v.y_station = rng.normal(size=4) * 0.2
    return v


@pytest.mark.parametrize("N,S,K", [(66, 40, 24), (130, 24, 16)])
def test_vi_gradients_returns_and_equals_the_numpy_chain_rules(N, S, K):
    """phylo_vi_gradients (refused above 65 taxa before) against Trainer(native=False): log Z-hat at the rtol 1e-12 of
    test_training_step_in_the_library_equals_the_numpy_step, and the gradients at that test's 1e-10 -- relative to the largest entry
    of their block, as every gradient check of the suite scales its error: the two sides differ by the last bit of exp() in the
    rates (libm against NumPy), which moves every entry by about 1e-16 of the block's scale, not of the entry's own size (one entry
    of 129 at 4e-3 in a block of 12 missed an element-wise 1e-10 by a factor 1.6 at N = 130; 5.6e-14 of the block).  The
    variables after two optimiser steps are compared element-wise, as that test does, in test_two_adam_steps_equal_the_numpy_trainer."""
    genome = coded_alignment(1000 + N, N, S)
    got = {}
    for native in (True, False):
        v = _variables(np.random.default_rng(21), N)
        tr = T.Trainer(genome, K, v, T.GradientDescent(0.0), S, native=native)
        try:
            if native:
                logZ, grads, raw, packed = tr._gradients_native(np.arange(S), 4)
                assert packed.shape == (2 * (N - 1) + 20,) and np.all(np.isfinite(packed))
            else:
                logZ, grads, raw = tr.gradients(np.arange(S), 4)
        finally:
            tr.close()
        got[native] = (logZ, grads)
    np.testing.assert_allclose(got[True][0], got[False][0], rtol=1e-12)
    for n in ('a_l', 'a_r', 'y_q', 'y_station'):
        scale = max(np.max(np.abs(got[False][1][n])), 1e-300)
        err = np.max(np.abs(got[True][1][n] - got[False][1][n])) / scale
        print('N %d %s native against NumPy: %.3e of the block' % (N, n, err))
        assert err < 1e-10, (n, err)


def test_vi_gradients_direct_call_twice_on_one_context():
    """The entry point itself at 66 taxa (PHYLO_EINVAL "at most 65 taxa" before): it returns, and a second step on the same context
    -- a second reverse pass -- gives the same bits."""
    N, S, K = 66, 40, 24
    v = _variables(np.random.default_rng(22), N)
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(coded_alignment(1000 + N, N, S))
        logZ, grads, fwd, bwd = ctx.vi_gradients(4, _ffi.FLAGS_DEFAULT, 1, False, v.pack())
        logZ2, grads2, _, _ = ctx.vi_gradients(4, _ffi.FLAGS_DEFAULT, 1, False, v.pack())   # a second pass on the context
    assert np.isfinite(logZ) and np.all(np.isfinite(grads)) and grads.shape == (2 * (N - 1) + 20,)
    assert logZ == logZ2 and np.array_equal(_bits(grads), _bits(grads2))
    assert bwd.n_launches > 0


def test_vi_gradients_batch_rows_equal_the_oracle_per_group():
    """G = 3 systems of K / G = 16 particles at N = 66: row g of phylo_vi_gradients_batch against the oracle of group g on the
    device's ancestors, through the oracle's own chain rules (to_variables), at 1e-9."""
    N, S, Kg, seeds = 66, 40, 16, [101, 102, 103]
    genome = coded_alignment(1000 + N, N, S)
    v = _variables(np.random.default_rng(23), N)
    Q, pi, ll, lr = v.evaluate()
    with _ffi.Context(Kg * len(seeds), N, S) as ctx:
        ctx.set_leaves(genome)
        z, grads, fwd, bwd = ctx.vi_gradients_batch(seeds, _ffi.FLAGS_DEFAULT, False, v.pack())
        z2, grads2, _, _ = ctx.vi_gradients_batch(seeds, _ffi.FLAGS_DEFAULT, False, v.pack())
        anc = ctx.sweep_fetch()['ancestors']
    assert np.array_equal(_bits(z), _bits(z2)) and np.array_equal(_bits(grads), _bits(grads2))
    for gi, sd in enumerate(seeds):
        ref = G.to_variables(Q, pi, ll, lr, _oracle(genome, Q, pi, ll, lr, Kg, sd, _ffi.FLAGS_DEFAULT, anc[:, gi * Kg:(gi + 1) * Kg]))
        mine = v.unpack_grads(grads[gi])
        for name, theirs in (('a_l', 'd_loglam_l'), ('a_r', 'd_loglam_r'), ('y_station', 'd_y_station'), ('y_q', 'd_y_q')):
            scale = max(np.max(np.abs(ref[theirs])), 1e-300)
            err = np.max(np.abs(mine[name] - ref[theirs])) / scale
            print('group %d %s rel err %.3e' % (gi, name, err))
            assert err < RTOL, (gi, name, err)


@pytest.mark.parametrize("N,S,K", [(66, 40, 24), (130, 24, 16)])
def test_two_adam_steps_equal_the_numpy_trainer(N, S, K):
    genome = coded_alignment(1000 + N, N, S)
    out = {}
    for native in (True, False):
        v = _variables(np.random.default_rng(24), N)
        tr = T.Trainer(genome, K, v, T.make_optimizer('Adam', 0.02), S, native=native)
        try:
            costs = [tr.step(np.arange(S), seed=30 + i) for i in range(2)]
        finally:
            tr.close()
        out[native] = (costs, {n: np.array(getattr(v, n)) for n in v.names()})
    np.testing.assert_allclose(out[True][0], out[False][0], rtol=1e-12)
    for n in out[True][1]:
        np.testing.assert_allclose(out[True][1][n], out[False][1][n], rtol=1e-10, atol=1e-13, err_msg=n)


def test_batched_and_nested_trainers_step_at_66_taxa():
    """Trainer(batched=3) and Trainer(nested=True) take a step each on 66 taxa: finite costs, variables moved."""
    N, S = 66, 16
    genome = coded_alignment(1000 + N, N, S)
    for kw, more in (({'batched': 3}, (8, 9)), ({'nested': True, 'M': 1}, ())):
        v = _variables(np.random.default_rng(25), N)
        a0 = v.a_l.copy()
        tr = T.Trainer(genome, 8, v, T.make_optimizer('Adam', 0.02), S, **kw)
        try:
            cost = tr.step(np.arange(S), 7, more)
        finally:
            tr.close()
        assert np.isfinite(cost) and not np.array_equal(v.a_l, a0) and np.all(np.isfinite(v.a_l)), kw


def test_vcsmc_train_one_epoch_on_80_taxa(tmp_path):
    from phylo_amd.vcsmc import VCSMC, default_args
    import random
    random.seed(3)
    args = default_args(n_particles=16, optimizer='Adam', learning_rate=0.05, batch_size=32, seed=7)
    v = VCSMC(datadict(1080, 80, 96), 16, args)
    lam0 = v.left_branches_param.copy()
    elbos = v.train(epochs=1, batch_size=32, learning_rate=0.05, save_dir=str(tmp_path))
    assert len(elbos) == 1 and np.all(np.isfinite(elbos))
    assert len(v.minibatch_costs) == 2 and np.all(np.isfinite(v.minibatch_costs))   # 96 sites: 3 slices, the last one skipped
    assert not np.array_equal(v.left_branches_param, lam0) and np.all(v.left_branches_param > 0)
    v.close()


# ---- 6. the twisted proposal -----------------------------------------------------------------------------------------------------------
def test_twisted_gradient_66_taxa_against_the_oracle():
    """N = 66, M = 1, K = 2, S = 8 against sweep_grad_twisted (oracle time: the module docstring)."""
    N, S, K = 66, 8, 2
    Q, pi, ll, lr = random_model(662, N)
    _check_twisted(coded_alignment(661, N, S), Q, pi, ll, lr, K=K, M=1, seed=5)


@pytest.mark.parametrize("N", [65, 100])
def test_twisted_pass_is_repeatable(N):
    """K = 8, M = 1: two passes with equal bits and finite values (no oracle: it would take minutes).  N = 100 is the issue's case;
    N = 65 is the smallest size that takes pk_twist_choose's form for more root slots than lanes (65 slots at rank event 0)."""
    S, K = 16, 8
    Q, pi, ll, lr = random_model(2000 + N, N)
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(coded_alignment(1000 + N, N, S))
        ctx.set_model(Q, pi, ll, lr)
        out = ctx.sweep(9, _ffi.FLAGS_DEFAULT | _ffi.TWISTING | _ffi.KEEP_GRAPH, 1)
        g, g2 = ctx.sweep_backward(), ctx.sweep_backward()
    assert np.isfinite(out['logZ'])
    _assert_same_bits(g, g2, 'twisted N %d' % N)
    assert all(np.all(np.isfinite(g[key])) for key in KEYS)
    assert np.any(g['d_lam_l'] != 0.0) and np.any(g['d_Q'] != 0.0)


# ---- 7. sharded --------------------------------------------------------------------------------------------------------------------------
def test_sharded_gradient_two_ranks_66_taxa():
    """Two processes (hostshm) share ONE 32-particle system on 66 taxa: the same gradient bits on both ranks and on the second
    pass, log Z-hat bit-identical to one GPU, the gradient within RTOL of the unsharded pass and of the oracle."""
    world, K, N, S, gen, seed = 2, 32, 66, 40, 1066, 11
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, PHYLO_RDZV_DIR=tmp, MASTER_PORT=str(29400 + (os.getpid() + 66) % 2000), PHYLO_COMM='hostshm')
        procs = []
        for r in range(world):
            path = os.path.join(tmp, "g%d.npz" % r)
            cmd = [sys.executable, os.path.join(ROOT, "tests", "_shard_grad_many_taxa_worker.py"), str(r), str(world), str(K), str(N), str(S),
                   str(gen), str(seed), path]
            procs.append((path, subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        outs = []
        for path, p in procs:
            try:
                log, _ = p.communicate(timeout=240)
            except subprocess.TimeoutExpired:
                for _, q in procs:
                    q.kill()
                raise
            assert p.returncode == 0, log.decode()[-3000:]
            outs.append(dict(np.load(path)))
    first = {k: outs[0]['%s_%d' % (k, seed)] for k in KEYS}
    for o in outs:
        assert o['logz_%d' % seed] == outs[0]['logz_%d' % seed]
        for k in KEYS:
            assert np.array_equal(_bits(o['%s_%d' % (k, seed)]), _bits(first[k])), k
            assert np.array_equal(_bits(o['again_%s_%d' % (k, seed)]), _bits(first[k])), k
    genome = coded_alignment(gen, N, S)
    Q, pi, ll, lr = random_model(gen + 1, N)
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(genome)
        ctx.set_model(Q, pi, ll, lr)
        ref = ctx.sweep(seed, _ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        one = ctx.sweep_backward()
    assert outs[0]['logz_%d' % seed] == ref['logZ']
    orc = _oracle(genome, Q, pi, ll, lr, K, seed, _ffi.FLAGS_DEFAULT, ref['ancestors'])
    _assert_oracle(first, ref['logZ'], orc, 'sharded N 66')
    _assert_oracle(first, ref['logZ'], dict(one, logZ=ref['logZ']), 'sharded against unsharded')
