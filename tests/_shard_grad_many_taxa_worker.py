"""One rank of a sharded reverse pass on a synthetic alignment (helper process of tests/test_gpu_grad_many_taxa.py;
tests/_shard_grad_worker.py takes its shape from a named dataset, and none has more than 64 taxa).
usage: python tests/_shard_grad_many_taxa_worker.py RANK WORLD K N S GEN_SEED SEEDS OUT.npz
Per seed: a sweep that keeps its graph, two reverse passes and the fetch."""
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

KEYS = ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q')


def main():
    rank, world, K, N, S, gen = (int(a) for a in sys.argv[1:7])
    seeds = [int(s) for s in sys.argv[7].split(',')]
    out = sys.argv[8]
    from phylo_amd import _ffi
    from phylo_amd.rendezvous import exchange_comm_id
    from tests.many_taxa_cases import coded_alignment, random_model
    g = coded_alignment(gen, N, S)
    Q, pi, ll, lr = random_model(gen + 1, N)
    ctx = _ffi.Context(K, N, S, device=0)
    ctx.set_leaves(g)
    ctx.set_model(Q, pi, ll, lr)
    cid = exchange_comm_id(rank, world, _ffi.comm_unique_id if rank == 0 else None)
    ctx.comm_init(rank, world, cid)
    res = {'k0': ctx.k0}
    for s in seeds:
        ctx.sweep_async(s, _ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        a = ctx.sweep_backward()
        b = ctx.sweep_backward()                           # the same kept graph again
        f = ctx.sweep_fetch()
        res['logz_%d' % s] = f['logZ']
        res['ancestors_%d' % s] = f['ancestors']
        for k in KEYS:
            res['%s_%d' % (k, s)] = a[k]
            res['again_%s_%d' % (k, s)] = b[k]
    np.savez(out, **res)
    ctx.close()


if __name__ == '__main__':
    main()
