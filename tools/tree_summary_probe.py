"""Device time of the tree posterior summary (phylo_tree_summary, hipEvents on the context's stream) against the host replay of
the same sweep in Python (VCSMC._final_tables + VCSMC.newick of the best particle), on one GPU.
python tools/tree_summary_probe.py [--reps 20]     one JSON line per case: primate.p K = 2048, DS1 K = 4096, 20 x 2048 batched
--branches: also the branch pass (phylo_tree_branches) after each summary, and the Python replay it replaces (_newick_table)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phylo_amd.datasets import load_dataset          # noqa: E402
from phylo_amd.vcsmc import VCSMC, default_args      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--branches', action='store_true')
a = ap.parse_args()


def device_ms(ctx, reps):
    ctx.tree_summary()                                # warm-up: code objects, the slab
    dev, wall = [], []
    for _ in range(reps):
        t = time.perf_counter()
        tab = ctx.tree_summary()
        wall.append((time.perf_counter() - t) * 1e3)
        dev.append(tab['summary_ms'])
    return float(np.median(dev)), float(np.median(wall)), tab


def branches_ms(ctx, tab, reps):
    ctx.tree_branches(tab)                            # warm-up: code objects, the slab
    dev, wall = [], []
    for _ in range(reps):
        t = time.perf_counter()
        b = ctx.tree_branches(tab)
        wall.append((time.perf_counter() - t) * 1e3)
        dev.append(b['branches_ms'])
    return float(np.median(dev)), float(np.median(wall)), b['branches_launches']


for name, dataset, Kg, G in (('primate_K2048', 'primate_data', 2048, 1), ('DS1_K4096', 'hohna_data_1', 4096, 1),
                             ('primate_20x2048', 'primate_data', 2048, 20)):
    d = load_dataset(dataset)
    v = VCSMC(d, K=Kg, args=default_args(seed=1))
    v.sample_phylogenies()
    t = time.perf_counter()
    v._final_tables()
    v.newick(int(np.argmax(v.log_likelihood_R)))
    host_ms = (time.perf_counter() - t) * 1e3 * G      # G independent sweeps replay G times
    t = time.perf_counter()
    if a.branches:
        v._newick_table()
    newick_ms = (time.perf_counter() - t) * 1e3 * G
    ctx = v._context()
    if G > 1:
        from phylo_amd import _ffi
        v.close()
        ctx = _ffi.Context(Kg * G, v.N, v.S)
        ctx.set_leaves(d['genome'])
        ctx.set_model(v.Qmatrix, v.stationary_probs, v.left_branches_param, v.right_branches_param)
        ctx.sweep_batch_async([1 + 10 * g for g in range(G)])
        ctx.synchronize()
    dev, wall, tab = device_ms(ctx, a.reps)
    extra = {}
    if a.branches:
        bdev, bwall, bl = branches_ms(ctx, tab, a.reps)
        extra = {'branches_device_ms': round(bdev, 4), 'branches_wall_ms': round(bwall, 4), 'branches_launches': bl,
                 'newick_table_ms': round(newick_ms, 2)}
    print(json.dumps({**extra, 'case': name, 'N': v.N, 'K': Kg * G, 'groups': G, 'summary_device_ms': round(dev, 4),
                      'summary_wall_ms': round(wall, 4), 'launches': tab['summary_launches'], 'clades': int(tab['clade_weight'].size),
                      'topologies': int(tab['topo_weight'].size), 'host_replay_ms': round(host_ms, 2),
                      'host_replay': '_final_tables + newick(best)' + (' x %d groups' % G if G > 1 else '')}), flush=True)
    if G > 1:
        ctx.close()
    else:
        v.close()
