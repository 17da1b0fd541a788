"""The merge that starts from the particle's merge record (pk_rank_merge_nostore, written to by every bookkeeping kernel):
bit for bit against the C oracle -- log-weights, log-likelihoods, merges, ancestors, log Z-hat -- at the smallest shapes at
which the record, its writers and the four child variants of the merge can go wrong."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import cpu_ref as O
from phylo_amd import _ffi
from phylo_amd.datasets import load_dataset, synthetic_alignment

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "merge_record_grad.npz")

PI = np.full((1, 4), 0.25)
EAGER = 1 | 8                                              # FLAGS_DEFAULT | PHYLO_EAGER_NODES


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(out, ref, what, sl=slice(None)):
    np.testing.assert_array_equal(out['ancestors'][:, sl], ref['ancestors'], err_msg=what)
    np.testing.assert_array_equal(out['merges'][:, sl], ref['merges'], err_msg=what)
    for key in ('log_weights', 'log_likelihood'):
        assert np.array_equal(bits(out[key][:, sl]), bits(ref[key])), "%s: %s differs" % (what, key)


def make_ctx(g, K, Q, pi=PI):
    N, S, _ = g.shape
    ctx = _ffi.Context(K, N, S)
    ctx.set_leaves(g)
    ctx.set_model(Q, pi, np.full(N - 1, 10.0), np.full(N - 1, 10.0))
    return ctx


def gtr():
    return O.get_Q(O.init_y_q())


@pytest.mark.parametrize("N", [4, 6])
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 130])
def test_odd_site_counts(N, S):
    """One valid lane, an odd number of 64-site steps, a last step with one valid lane."""
    g = synthetic_alignment(N, S, seed=7 * N + S)['genome']
    lam = np.full(N - 1, 10.0)
    Q, pi = gtr(), np.array([[0.1, 0.2, 0.3, 0.4]])
    ctx = make_ctx(g, 64, Q, pi)
    out = ctx.sweep(5)
    ref = CO.sweep(g, Q, pi, lam, lam, 64, 5)
    same(out, ref, "N=%d S=%d" % (N, S))
    assert out['logZ'] == ref['logZ']
    ctx.close()


def test_four_child_variants(monkeypatch):
    """Coded x coded, coded x rows, rows x coded and rows x rows in one sweep (leaves merge with leaves and with nodes); the
    same alignment with one row that is neither one-hot nor all-ones (no codes: every row the generic way), and with the codes
    switched off."""
    N, S, K = 6, 66, 64
    g = synthetic_alignment(N, S, seed=3)['genome']
    g[2, 10] = 1.0                                         # an all-ones row: code 4
    lam = np.full(N - 1, 10.0)
    Q, pi = gtr(), np.array([[0.4, 0.3, 0.2, 0.1]])
    ref = CO.sweep(g, Q, pi, lam, lam, K, 9)
    ctx = make_ctx(g, K, Q, pi)
    out = ctx.sweep(9)
    same(out, ref, "codes")
    assert out['logZ'] == ref['logZ']
    ctx.close()
    monkeypatch.setenv("PHYLO_NO_LEAF_CODES", "1")
    ctx = make_ctx(g, K, Q, pi)
    out = ctx.sweep(9)
    same(out, ref, "codes switched off")
    assert out['logZ'] == ref['logZ']
    ctx.close()
    monkeypatch.delenv("PHYLO_NO_LEAF_CODES")
    h = g.copy()
    h[1, 5] = [0.5, 0.5, 0.0, 0.0]                         # neither one-hot nor all-ones: the alignment has no codes
    ref = CO.sweep(h, Q, pi, lam, lam, K, 9)
    ctx = make_ctx(h, K, Q, pi)
    out = ctx.sweep(9)
    same(out, ref, "no codes")
    assert out['logZ'] == ref['logZ']
    ctx.close()


def test_more_than_one_tile():
    """S = 130 in tiles of 64: the merge leaves tile values, pk_tile_epilogue finishes the particle."""
    N, S, K = 5, 130, 64
    g = synthetic_alignment(N, S, seed=11)['genome']
    lam = np.full(N - 1, 10.0)
    Q = gtr()
    ctx = make_ctx(g, K, Q)
    ctx.set_site_tile(64)
    CO.set_site_tile(64)
    try:
        ref = CO.sweep(g, Q, PI, lam, lam, K, 3)
        out = ctx.sweep(3)
        same(out, ref, "tiles")
        assert out['logZ'] == ref['logZ']
    finally:
        CO.set_site_tile(0)
        ctx.close()


def test_batched_groups_equal_single_sweeps():
    """G = 3 groups of 64: the record's destinations are global columns."""
    N, S, G, Kg = 6, 66, 3, 64
    g = synthetic_alignment(N, S, seed=2)['genome']
    lam = np.full(N - 1, 10.0)
    Q = gtr()
    seeds = [4, 90, 17]
    ctx = make_ctx(g, G * Kg, Q)
    ctx.sweep_batch_async(seeds)
    out = ctx.sweep_fetch()
    logz = ctx.sweep_fetch_logz(G)
    for i, s in enumerate(seeds):
        ref = CO.sweep(g, Q, PI, lam, lam, Kg, s)
        same(out, ref, "group %d" % i, slice(i * Kg, (i + 1) * Kg))
        assert logz[i] == ref['logZ']
    ctx.close()


@pytest.mark.parametrize("N,G,Kg,writer", [
    (6, 1, 64, "pk_rank_book_mat"),                        # one sweep, lazy nodes, N <= 64
    (4, 2, 4096, "pk_rank_book_packed<8>"),                # N <= 16 and 8192 particles, batched (no pk_rank_book_mat)
    (33, 2, 32, "pk_rank_book_packed<64>"),                # more than 32 taxa, batched
])
def test_every_bookkeeping_writer(N, G, Kg, writer):
    """Each kernel that writes the record; lazy nodes equal eager nodes (which merge from ids, with the storing kernel)."""
    S = 66
    g = synthetic_alignment(N, S, seed=N)['genome']
    lam = np.full(N - 1, 10.0)
    Q = gtr()
    seeds = [21, 22][:G]
    ctx = make_ctx(g, G * Kg, Q)
    outs, logzs = [], []
    for flags in (1, EAGER):
        if G == 1:
            outs.append(ctx.sweep(seeds[0], flags=flags))
            logzs.append([outs[-1]['logZ']])
        else:
            ctx.sweep_batch_async(seeds, flags=flags)
            outs.append(ctx.sweep_fetch())
            logzs.append(list(ctx.sweep_fetch_logz(G)))
    ctx.close()
    for key in ('log_weights', 'log_likelihood'):
        assert np.array_equal(bits(outs[0][key]), bits(outs[1][key])), "%s: lazy %s differs from eager" % (writer, key)
    np.testing.assert_array_equal(outs[0]['ancestors'], outs[1]['ancestors'])
    np.testing.assert_array_equal(outs[0]['merges'], outs[1]['merges'])
    assert outs[0]['logZ'] == outs[1]['logZ']
    for i, sd in enumerate(seeds):                          # every group's destination columns, both forms
        ref = CO.sweep(g, Q, PI, lam, lam, Kg, sd)
        for out, form in zip(outs, ("lazy", "eager")):
            same(out, ref, "%s %s group %d" % (writer, form, i), slice(i * Kg, (i + 1) * Kg))
        assert logzs[0][i] == ref['logZ'] and logzs[1][i] == ref['logZ']


def _two_ranks(extra_env, K, dataset, seed):
    """Two processes on GPU 0 over hostshm (tests/_shard_worker.py); each child under its own time limit."""
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, PHYLO_RDZV_DIR=tmp, MASTER_PORT=str(31000 + os.getpid() % 2000), PHYLO_COMM='hostshm')
        env.update(extra_env)
        procs = []
        for r in range(2):
            out = os.path.join(tmp, "r%d.npz" % r)
            procs.append((out, subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_shard_worker.py"), str(r), '2', str(K),
                                                 dataset, str(seed), '0', out, '1'], env=env, stdout=subprocess.PIPE,
                                                stderr=subprocess.STDOUT)))
        outs = []
        for out, p in procs:
            try:
                log, _ = p.communicate(timeout=120)
            except subprocess.TimeoutExpired:
                for _, q in procs:
                    q.kill()
                raise
            if p.returncode != 0:
                for _, q in procs:
                    q.kill()
            assert p.returncode == 0, log.decode()[-2000:]
            outs.append(dict(np.load(out)))
        return outs


def test_two_ranks_on_one_gpu():
    """Sharded sweeps merge from ids (pk_rank_merge_nostore_ids: a remote child's address is not in a record): remote cache on,
    cache full (children read in place), cache off -- each against the oracle, stopping at the first failure."""
    dataset, K, seed = 'primate_data', 64, 4
    g = load_dataset(dataset)['genome']
    N = g.shape[0]
    lam = np.full(N - 1, 10.0)
    Q = gtr()
    ref = CO.sweep(g, Q, PI, lam, lam, K, seed)
    Kl = K // 2
    for env in ({}, {'PHYLO_REMOTE_CACHE_CAP': '1'}, {'PHYLO_NO_REMOTE_CACHE': '1'}):
        parts = _two_ranks(env, K, dataset, seed)
        for r, p in enumerate(parts):
            sl = slice(r * Kl, (r + 1) * Kl)
            what = "%r rank %d" % (env, r)
            np.testing.assert_array_equal(p['ancestors'], ref['ancestors'][:, sl], err_msg=what)
            np.testing.assert_array_equal(p['merges'], ref['merges'][:, sl], err_msg=what)
            for key in ('log_weights', 'log_likelihood'):
                assert np.array_equal(bits(p[key]), bits(ref[key][:, sl])), "%s: %s differs" % (what, key)
            assert float(p['logZ']) == ref['logZ'], what
        assert (parts[0]['ancestors'] >= Kl).any()          # remote children were merged


def grad_case():
    """One kept-graph sweep and its reverse pass: K = 64, N = 6, S = 66."""
    g = synthetic_alignment(6, 66, seed=5)['genome']
    ctx = make_ctx(g, 64, gtr(), np.array([[0.1, 0.2, 0.3, 0.4]]))
    out = ctx.sweep(13, _ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
    grad = ctx.sweep_backward()
    ctx.close()
    res = {k: np.asarray(v) for k, v in grad.items() if k.startswith('d_')}
    res['logZ'] = np.asarray(out['logZ'])
    return res


def test_kept_graph_gradient_equals_recorded_value():
    """The reverse pass reads child_all, which the bookkeeping writes beside the record: the gradient of one training step has
    the bits recorded (tests/golden/merge_record_grad.npz) from the commit before the record existed."""
    want = np.load(GOLDEN)
    got = grad_case()
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert np.array_equal(bits(got[k]), bits(want[k])), "%s differs from the recorded gradient" % k
