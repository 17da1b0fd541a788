"""One rank of a sharded reverse pass (helper process of tests/test_gpu_sharded_grad.py).
usage: python tests/_shard_grad_worker.py RANK WORLD K DATASET JC MODE SEEDS OUT.npz
MODE grad: per seed, a sweep that keeps its graph, two reverse passes and the fetch; node: per seed, the reverse pass of a lazy
kept graph, then of the same sweep after phylo_sweep_node (which writes every node the lazy sweep skipped); vi: a sequence of phylo_vi_gradients +
phylo_vi_apply (Adam) steps, one per seed; refuse: the refused calls, then one plain sweep."""
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

KEYS = ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q')


def main():
    rank, world, K = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    dataset, jc, mode = sys.argv[4], sys.argv[5] == '1', sys.argv[6]
    seeds = [int(s) for s in sys.argv[7].split(',')]
    out = sys.argv[8]
    from phylo_amd import _ffi, model
    from phylo_amd.datasets import load_dataset
    from phylo_amd.rendezvous import exchange_comm_id
    g = load_dataset(dataset)['genome']
    N, S, _ = g.shape
    Q = model.jc_Q() if jc else model.get_Q(model.init_y_q())
    pi = model.get_stationary_probs(np.zeros(4) + 0.25)
    lam = np.full(N - 1, 10.0)
    ctx = _ffi.Context(K, N, S, device=0)
    ctx.set_leaves(g)
    ctx.set_model(Q, pi, lam, lam, jc69_closed_form=jc)
    cid = exchange_comm_id(rank, world, _ffi.comm_unique_id if rank == 0 else None)
    ctx.comm_init(rank, world, cid)
    res = {'k0': ctx.k0}
    flags = _ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH
    if mode == 'grad':
        for s in seeds:
            ctx.sweep_async(s, flags)
            a = ctx.sweep_backward()
            b = ctx.sweep_backward()                       # the same kept graph again
            f = ctx.sweep_fetch()
            res['logz_%d' % s] = f['logZ']
            for k in KEYS:
                res['%s_%d' % (k, s)] = a[k]
                res['again_%s_%d' % (k, s)] = b[k]
    elif mode == 'node':
        for s in seeds:
            ctx.sweep_async(s, flags)
            a = ctx.sweep_backward()
            ctx.sweep_async(s, flags)
            ctx.sweep_node(2, 5)                           # a collective on a sharded context
            b = ctx.sweep_backward()
            for k in KEYS:
                res['%s_%d' % (k, s)] = a[k]
                res['node_%s_%d' % (k, s)] = b[k]
    elif mode == 'vi':
        v = np.concatenate([np.full(2 * (N - 1), np.log(10.0)), model.init_y_q().reshape(-1), np.zeros(4)])
        state = {'t': 0, 'm': np.zeros_like(v), 'v': np.zeros_like(v)}
        for i, s in enumerate(seeds):
            logz, grads, _, _ = ctx.vi_gradients(s, _ffi.FLAGS_DEFAULT, 1, jc, v)
            res['logz_%d' % i] = logz
            res['grads_%d' % i] = grads.copy()
            _ffi.vi_apply(N, jc, v, grads, 1, 0.05, state=state)
            res['vars_%d' % i] = v.copy()
    elif mode == 'refuse':
        codes = {}
        for name, fl in (('twisted', flags | _ffi.TWISTING), ('backward', None)):
            try:
                if fl is None:
                    ctx.sweep(seeds[0], _ffi.FLAGS_DEFAULT)        # no kept graph
                    ctx.sweep_backward()
                else:
                    ctx.sweep_async(seeds[0], fl, 2)
                codes[name] = 0
            except _ffi.PhyloError as e:
                codes[name] = e.code
        for name, c in codes.items():
            res['code_' + name] = c
        f = ctx.sweep(seeds[0], _ffi.FLAGS_DEFAULT)
        res['logz'] = f['logZ']
        res['log_weights'] = f['log_weights']
        # more than 4096 sites per context
        wide = np.tile(g, (1, 4096 // S + 1, 1))
        big = _ffi.Context(K, N, wide.shape[1], device=0)
        big.set_leaves(wide)
        big.set_model(Q, pi, lam, lam, jc69_closed_form=jc)
        big.comm_share(ctx)
        try:
            big.sweep_async(seeds[0], flags)
            res['code_wide'] = 0
        except _ffi.PhyloError as e:
            res['code_wide'] = e.code
        big.close()
    np.savez(out, **res)
    ctx.close()


if __name__ == '__main__':
    main()
