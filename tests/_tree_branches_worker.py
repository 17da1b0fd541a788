"""One rank of a sharded sweep followed by its tree posterior summary and branch pass (helper process of
tests/test_gpu_tree_branches.py and tests/test_gpu_tree_branches_wide.py; the saved 'branch_plan' is (wide, cbits, tbits) of the
pass, phylo_debug_tree_branches_of).
usage: python tests/_tree_branches_worker.py RANK WORLD K DATASET SEED KEEP_GRAPH OUT.npz"""
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    rank, world, K = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    dataset, seed, keep, out = sys.argv[4], int(sys.argv[5]), int(sys.argv[6]), sys.argv[7]
    from phylo_amd import _ffi, model
    from phylo_amd.datasets import load_dataset
    from phylo_amd.rendezvous import exchange_comm_id
    g = load_dataset(dataset)['genome']
    N, S, _ = g.shape
    lam = np.full(N - 1, 10.0)
    ctx = _ffi.Context(K, N, S, device=int(os.environ.get('PHYLO_TEST_DEVICE', '0')))
    ctx.set_leaves(g)
    ctx.set_model(model.jc_Q(), np.full((1, 4), 0.25), lam, lam, jc69_closed_form=True)
    cid = exchange_comm_id(rank, world, _ffi.comm_unique_id if rank == 0 else None)
    ctx.comm_init(rank, world, cid)
    ctx.sweep(seed, flags=_ffi.FLAGS_DEFAULT | (_ffi.KEEP_GRAPH if keep else 0))
    tab = ctx.tree_summary()
    tab.update(ctx.tree_branches(tab))
    plan = ctx.debug_tree_branches()
    tab['branch_plan'] = np.array([int(plan['wide']), plan['cbits'], plan['tbits']], dtype=np.int32)
    np.savez(out, **{k: v for k, v in tab.items() if isinstance(v, np.ndarray)})
    ctx.close()


if __name__ == '__main__':
    main()
